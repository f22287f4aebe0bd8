"""The 256^2 GEMM's fused per-segment column statistics (csrc/conv_gemm.hip: tile_stats, the half-tile tail's zero slot,
colstats_finish_kernel) against the EXACT sums of tests/colstats_ref.py, at every geometry class of the epilogue.

The test owns the buffers (sdk_conv_gemm / sdk_colstats_finish through ctypes):
  * stats_part is sdk_conv_gemm_stats_bytes + a guard tail, every byte 0xFF.  A float of all-ones bits is a NaN, so a slot the finish kernel
    reads but the GEMM never wrote shows as a NaN statistic; the guard tail must stay 0xFF.
  * C has 256 guard rows behind it, filled with a sentinel, which must be unchanged.

What is asserted, per case (colstats_ref.operands: small integers, ReLU, scale in {0.5, 1, 2}, every 64th column all zero):
  * output: the bits of the reference (exact in bf16 / fp16).
  * mean: bit-equal to float32(s) * (float32(1) / float32(T)) in numpy float32.  s is exact (colstats_ref.exact_conditions: every fp32
    partial sum in any order is exact), so these are the kernel's two IEEE operations.  The division is the correctly rounded one: the
    gfx950 code of colstats_finish_kernel (hipcc -O3, no fast-math, read from the cross-compiled assembly) is v_div_scale_f32 x 2, v_rcp_f32,
    the v_fma_f32 refinement, v_div_fmas_f32 and v_div_fixup_f32 - not a bare v_rcp_f32 - followed by v_mul_f32 for the mean.
  * std (mode 2): q and s are exact.  The kernel's q * invT - mean^2 is at most three fp32 roundings of quantities no larger than
    m = max(q / T, mean^2) under any FMA contraction (the assembly shows none: one v_pk_mul_f32 for both products, one v_sub_f32), then one
    correctly rounded square root (v_sqrt_f32 plus the two-sided fix-up).  So |sd_gpu - sd_exact| <= 3 * 2^-24 * m / sd_exact + 2^-24 * sd_exact,
    doubled for the roundings invT and mean already carry (colstats_ref.std_bound; no measured constant).  Fixture condition, on the
    reference alone: every ordinary column of every segment has exact variance >= 1.  The all-zero columns give exactly
    float32(sqrt(float32(1e-12))), the variance floor.
  * determinism: a second run on fresh buffers gives the same bits, output and statistics.
Each case prints its shape and geometry classes, the worst std error and that error's bound before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import colstats_ref as R
from conftest import sub

pytestmark = pytest.mark.gpu

L = sub("_lib")

GUARD_ROWS = 256
PART_GUARD = 4096                    # bytes behind stats_part
SENTINEL = 0x7B7B                    # two-byte pattern of the guard rows (bf16 1.3e36, fp16 61280: no case produces either)
STD_FLOOR = np.sqrt(np.float32(R.VAR_FLOOR))
assert STD_FLOOR.dtype == np.float32


class _Buffers:
    def __init__(self, eng, M, N, T, mode, dtype):
        self.nbytes = eng.lib.sdk_conv_gemm_stats_bytes(M, N, mode)
        assert self.nbytes == ((M + 255) // 256) * 6 * N * 4 * mode
        self.c = torch.full((M * N + GUARD_ROWS * N,), SENTINEL, dtype=torch.int16, device="cuda")
        self.part = torch.full((self.nbytes + PART_GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        self.st = torch.full((M // T if M % T == 0 else 1, N * mode), float("nan"), dtype=torch.float32, device="cuda")
        self.M, self.N, self.dtype = M, N, dtype

    def untouched(self):
        return bool((self.c == SENTINEL).all()) and bool((self.part == 0xFF).all()) and bool(torch.isnan(self.st).all())

    def guards_ok(self):
        return bool((self.c[self.M * self.N:] == SENTINEL).all()), bool((self.part[self.nbytes:] == 0xFF).all())


def _args(buf, A, Wt, o, T, taps, dil, mode, flags, N=None, M=None):
    g = L.ConvGemmArgs()
    g.A, g.lda, g.W, g.C, g.ldc = A.data_ptr(), A.stride(0), Wt.data_ptr(), buf.c.data_ptr(), N or buf.N
    g.bias, g.scale, g.shift = o["bias"].data_ptr(), o["scale"].data_ptr(), o["shift"].data_ptr()
    g.M, g.N, g.Cin, g.taps, g.dil, g.T = M or buf.M, N or buf.N, R.CIN, taps, dil, T
    g.flags = flags
    g.stats_mode, g.stats_part = mode, buf.part.data_ptr()
    return g


def _device_operands(o, fmt):
    dt = R.DTYPES[fmt]
    d = {k: o[k].cuda() for k in ("bias", "scale", "shift")}
    return o["A"].to(dt).cuda(), o["Wt"].to(dt).cuda(), d


def _run(eng, o, fmt, mode, taps=1, dil=1, kblocked=False):
    """one GEMM + finish on fresh prefilled buffers -> (output bits int16 [M, N], statistics float32 [B, N * mode]), both on the CPU"""
    M, N, T = o["M"], o["N"], o["T"]
    A, Wt, d = _device_operands(o, fmt)
    buf = _Buffers(eng, M, N, T, mode, R.DTYPES[fmt])
    flags = L.GEMM_RELU | (L.GEMM_F16 if fmt == "fp16" else 0) | (L.GEMM_C_KBLOCKED if kblocked else 0)
    g = _args(buf, A, Wt, d, T, taps, dil, mode, flags)
    s = torch.cuda.current_stream().cuda_stream
    L.check(eng.lib.sdk_conv_gemm(eng.ctx, C.byref(g), s), "sdk_conv_gemm")
    L.check(eng.lib.sdk_colstats_finish(eng.ctx, buf.part.data_ptr(), M, N, T, mode, buf.st.data_ptr(), s), "sdk_colstats_finish")
    torch.cuda.synchronize()
    c_guard, part_guard = buf.guards_ok()
    assert c_guard, "the guard rows behind C were written"
    assert part_guard, "the guard tail behind stats_part was written"
    c = buf.c[:M * N]
    if kblocked:
        c = eng.from_kblocked(c.view(N // 64, M, 64))
    return c.reshape(M, N).cpu(), buf.st.cpu()


def _check(o, ref, fmt, mode, bits, st, what):
    """print the figures, then assert output, mean and std of one run against the exact reference"""
    M, N, T = o["M"], o["N"], o["T"]
    a, q, exact = R.exact_conditions(ref)
    got = st.numpy()
    mean = R.expected_mean(ref)
    nan = int(np.isnan(got).sum())
    keep = np.ones(N, dtype=bool)
    keep[o["zero"].numpy()] = False
    line = f"{what}: M={M} T={T} N={N} {fmt} mode {mode}, classes {sorted(R.geometry(M, T), key=str)}; NaN statistics {nan}; mean mismatches {int((got[:, :N] != mean).sum())}"
    if mode == 2:
        sd = ref.std.numpy()
        err = np.abs(got[:, N:].astype(np.float64) - sd)[:, keep]
        bound = R.std_bound(ref).numpy()[:, keep]
        with np.errstate(invalid="ignore"):
            ratio = np.where(np.isnan(err), np.inf, err / bound)
        k = np.unravel_index(np.argmax(ratio), ratio.shape)
        line += f"; worst std error {err[k]:.3e} against its bound {bound[k]:.3e} (ratio {ratio[k]:.3f}), min exact variance {float(sd[:, keep].min()) ** 2:.3f}"
    print(line)
    assert exact, f"fixture: sum|v| = {a}, sum v^2 = {q} quanta, not below 2^24"
    assert nan == 0, f"{nan} statistics are NaN: a stats_part slot was read but never written"
    assert torch.equal(bits, ref.out.to(R.DTYPES[fmt]).view(torch.int16)), "output differs from the exact reference"
    assert np.array_equal(got[:, :N].view(np.int32), mean.view(np.int32)), f"mean: {int((got[:, :N] != mean).sum())} of {mean.size} differ from the exact sums"
    if mode == 2:
        assert float(sd[:, keep].min()) >= 1.0, "fixture: an ordinary column with exact variance below 1"
        assert not ref.out[:, o["zero"]].any()
        assert np.array_equal(got[:, N:][:, ~keep].view(np.int32), np.full((M // T, int((~keep).sum())), STD_FLOOR).view(np.int32)), "all-zero columns: not the variance floor"
        assert float(ratio.max()) <= 1.0, f"std error {err[k]} above its derived bound {bound[k]}"


def _twice(eng, o, ref, fmt, mode, what, **kw):
    bits, st = _run(eng, o, fmt, mode, **kw)
    _check(o, ref, fmt, mode, bits, st, what)
    bits2, st2 = _run(eng, o, fmt, mode, **kw)
    assert torch.equal(bits, bits2) and torch.equal(st.view(torch.int32), st2.view(torch.int32)), "two runs differ"


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("T,B", R.SHAPES)
def test_colstats_exact_at_every_geometry_class(engine, T, B, fmt, mode):
    """a. every row of the shared table, N = 512 (two column tiles: the n0 offset), taps = 1"""
    o, ref = R.case(T, B, 512, fmt=fmt)
    _twice(engine, o, ref, fmt, mode, "a")


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("T,B", [(129, 34), (160, 5)])
def test_colstats_exact_with_conv_taps(engine, T, B, fmt):
    """b. taps = 3, dil = 2: the <CONV = true> instantiation (reflected row gather), mode 2"""
    o, ref = R.case(T, B, 512, taps=3, dil=2, fmt=fmt)
    _twice(engine, o, ref, fmt, 2, "b", taps=3, dil=2)


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("T,B", [(129, 34), (255, 3)])
def test_colstats_exact_with_kblocked_output(engine, T, B, fmt):
    """c. SDK_GEMM_C_KBLOCKED: statistics against the reference (not against the row-major schedule), from_kblocked(C) against the
    reference output"""
    o, ref = R.case(T, B, 512, fmt=fmt)
    _twice(engine, o, ref, fmt, 2, "c", kblocked=True)


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_colstats_exact_when_workgroups_reuse_their_lds_buffers(engine, fmt):
    """d. more tiles than compute units: the persistent workgroups (one per CU) walk more than one tile, so tile_stats runs again on the same
    per-wave LDS partials behind its barriers.  (T, B) = (129, 34): 18 row tiles x N / 256 column tiles."""
    T, B, N = 129, 34, 4096
    cus = L.device_info(0)["compute_units"]
    tiles = lambda n: ((T * B + 255) // 256) * (n // 256)
    while tiles(N) <= cus:
        N += 256
    print(f"d: {tiles(N)} tiles on {cus} compute units")
    assert tiles(N) > cus
    o, ref = R.case(T, B, N, fmt=fmt)
    _twice(engine, o, ref, fmt, 2, "d")


def test_colstats_exact_in_the_half_tile_tail_and_without_it(engine):
    """e. M = 40200 = 200 x 201, N = 1024: with the half-tile tail (gemm variant 2; the last tile's lower half is wholly below the matrix: the
    zero-slot branch) and as whole tiles only (8194), each against the reference - not against each other"""
    o, ref = R.case(201, 200, 1024, fmt="bf16")
    try:
        for v in (2, 8194):
            engine.lib.sdk_set_gemm_variant(v)
            bits, st = _run(engine, o, "bf16", 2)
            _check(o, ref, "bf16", 2, bits, st, f"e (gemm variant {v})")
    finally:
        engine.lib.sdk_set_gemm_variant(2)


def test_colstats_refusals_launch_nothing(engine):
    """f. shapes the fused statistics do not cover are refused with the existing messages, sdk_conv_gemm_stats_fusable agrees, nothing is
    written, and a good call afterwards passes"""
    lib, s = engine.lib, torch.cuda.current_stream().cuda_stream
    need = "fused column statistics need the 256^2 kernel"
    o, ref = R.case(128, 3, 512, fmt="bf16")
    A, Wt, d = _device_operands(o, "bf16")
    A = torch.cat([A, A[:1]])                  # 385 rows: every M below is inside it
    buf = _Buffers(engine, 384, 512, 128, 2, torch.bfloat16)
    for M, N, T, mode, null_part, msg in [(381, 512, 127, 2, False, need), (255, 512, 255, 1, False, need), (384, 128, 128, 2, False, need),
                                          (384, 512, 128, 2, True, need), (384, 512, 128, 3, False, "stats_mode=3")]:
        g = _args(buf, A, Wt, d, T, 1, 1, mode, L.GEMM_RELU, N=N, M=M)
        if null_part:
            g.stats_part = None
        rc = lib.sdk_conv_gemm(engine.ctx, C.byref(g), s)
        text = lib.sdk_last_error().decode()
        print(f"f: M={M} N={N} T={T} mode={mode} null={null_part}: rc {rc}, '{text}'")
        assert rc != 0 and msg in text
        if not null_part and mode != 3:
            assert lib.sdk_conv_gemm_stats_fusable(M, N, T) == 0
    assert lib.sdk_conv_gemm_stats_fusable(384, 512, 128) == 1
    rc = lib.sdk_colstats_finish(engine.ctx, buf.part.data_ptr(), 385, 512, 128, 2, buf.st.data_ptr(), s)
    assert rc != 0 and "sdk_colstats_finish: bad shape" in lib.sdk_last_error().decode()
    torch.cuda.synchronize()
    assert buf.untouched(), "a refused call wrote to its buffers"
    bits, st = _run(engine, o, "bf16", 2)
    _check(o, ref, "bf16", 2, bits, st, "f (a good call after the refusals)")
