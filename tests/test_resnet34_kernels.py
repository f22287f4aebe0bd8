"""Kernel-level parity of the ResNet34 family (csrc/resnet.hip, sdk_resnet_forward), beside the model-level tests of test_resnet34.py.
CPU: pick_tile restated, and the integer sweep's coverage of every tile shape, kernel instance and edge map.  GPU: sdk_resnet_conv2d bit-exact on
small-integer operands over that sweep (bf16 and fp16, ReLU on and off, the stem); real-valued operands against float64 at a storage-ulp bound and
the fp16 saturation; the 33 convs of sdk_resnet_forward replayed one by one at production shapes, each against float64 of its own stored inputs,
and the forward's embedding against the float64 pooling of the replayed last map times seg_1; the Backend's default batch of 5-s windows; the
refusals of sdk_resnet_conv2d and sdk_resnet_forward."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import sub
import resnet_ref as RR

RN = sub("resnet")
LIB = sub("_lib")

U32 = 2.0 ** -24                                  # fp32 unit roundoff
SENTINEL = 777.0


# ------------------------------------------------------------------------------------------------------------------------------- CPU
def pick_tile(Fo, To, s):
    """resnet.hip pick_tile: the R x W position tile (R W = 64) with the fewest computed positions, then the smallest LDS patch."""
    best = None
    for w in (8, 16, 32, 64):
        r = 64 // w
        key = (-(-Fo // r) * -(-To // w) * 64, ((r - 1) * s + 3) * ((w - 1) * s + 3))
        if best is None or key < best[0]:
            best = (key, (r, w))
    return best[1]


def _out(n, s):
    return (n - 1) // s + 1


PROD_T = (9, 51, 101, 151, 201, 301, 501)         # segment lengths in frames: 0.1 .. 5 s windows
PROD_LAYERS = [(32, 32, 1, 80), (32, 64, 2, 80), (64, 64, 1, 40), (64, 128, 2, 40), (128, 128, 1, 20), (128, 256, 2, 20), (256, 256, 1, 10)]


def _prod_in_T(T, F):
    """The frames of the production map of height F at segment length T."""
    for f, t in RN.DEFAULT_RESNET.map_sizes(T):
        if f == F:
            return t
    raise ValueError(F)


# (Cin, Cout, stride, F, T, relu) of the integer sweep; a same-width stride-1 case carries its identity residual.  B = 3 segments each.
CONV_GRID = [
    # production layer shapes at production maps (T = 201 and 501 chains; T = 9 for the 2-frame layer-4 map)
    (32, 32, 1, 80, 51, True),      # layer1 at T = 51: 8x8
    (32, 64, 2, 80, 201, True),     # layer2.0.conv1: 40 x 101 out, 8x8
    (64, 64, 1, 40, 101, True),     # layer2 identity: 8x8
    (64, 128, 2, 40, 101, True),    # layer3.0.conv1: 20 x 51 out, 4x16
    (128, 128, 1, 20, 51, True),    # layer3 identity: 4x16, NTILE = 128 with its residual
    (128, 128, 1, 20, 13, False),   # layer3 identity at T = 51: 4x16, ReLU off
    (128, 256, 2, 20, 51, True),    # layer4.0.conv1: 10 x 26 out, 2x32
    (128, 256, 2, 20, 126, False),  # layer4.0.conv1 at T = 501: 10 x 63 out, 2x32
    (256, 256, 1, 10, 63, True),    # layer4 identity at T = 501: 2x32
    (256, 256, 1, 10, 2, True),     # layer4 identity at T = 9: a 2-frame map
    # the remaining kernel instances, tile shapes and edge maps
    (256, 32, 1, 1, 40, False),     # 1x64 at stride 1, Fo = 1
    (64, 256, 1, 1, 70, True),      # 1x64 at stride 1, two tiles along t
    (32, 128, 1, 3, 17, True),      # 4x16 at stride 1
    (32, 256, 1, 2, 33, False),     # 2x32 at stride 1
    (32, 64, 1, 1, 2, True),        # Fo = 1, To = 2
    (128, 128, 1, 1, 1, False),     # Fo = To = 1 with its residual
    (32, 32, 2, 1, 1, True),        # stride 2, Fo = To = 1
    (64, 32, 2, 2, 100, False),     # 1x64 at stride 2 (1 x 50 out)
    (128, 64, 2, 2, 130, True),     # 1x64 at stride 2, two tiles along t (1 x 65 out)
    (32, 256, 2, 1, 66, True),      # 1x64 at stride 2, CK = 32
    (32, 128, 2, 3, 3, False),      # stride 2, 2 x 2 out
    (32, 256, 2, 3, 17, True),      # 4x16 at stride 2 (2 x 9 out), CK = 32
    (64, 64, 2, 3, 64, True),       # 2x32 at stride 2 (2 x 32 out)
    (256, 32, 2, 9, 17, False),     # 8x8 at stride 2 (5 x 9 out)
]


def _has_res(Cin, Cout, s):
    return Cin == Cout and s == 1


def _case_id(c):
    Cin, Cout, s, F, T, relu = c
    return f"{Cin}-{Cout}-s{s}-{F}x{T}" + ("" if relu else "-norelu")


def test_integer_sweep_covers_every_tile_shape_kernel_instance_and_edge_map():
    """The sweep below drives every R x W tile at both strides, every resnet_conv_kernel<NTILE, S, CK, F16> dispatch_conv can launch (F16 by the
    test's parametrisation), the layer-3 identity block with its residual, maps of one row / one or two frames, both ReLU settings, and every
    production layer shape at a production map.  Editing the grid or the heuristic so that a case drops out fails here."""
    # the restated heuristic picks what the production tiles are known to be
    assert pick_tile(20, 51, 1) == (4, 16) and pick_tile(10, 26, 2) == (2, 32) and pick_tile(80, 201, 1) == (8, 8)
    tiles, insts = set(), set()
    for Cin, Cout, s, F, T, relu in CONV_GRID:
        tiles.add((pick_tile(_out(F, s), _out(T, s), s), s))
        insts.add((Cout, s, 32 if Cin == 32 else 64))
    assert tiles == {((r, 64 // r), s) for r in (8, 4, 2, 1) for s in (1, 2)}, tiles
    assert insts == {(n, s, ck) for n in (32, 64, 128, 256) for s in (1, 2) for ck in (32, 64)}, insts
    assert any(c[:3] == (128, 128, 1) for c in CONV_GRID)
    assert {c[5] for c in CONV_GRID} == {True, False}
    outs = [(_out(c[3], c[2]), _out(c[4], c[2])) for c in CONV_GRID]
    assert (1, 1) in outs and (1, 2) in outs and any(fo == 1 and to > 64 for fo, to in outs)
    for Cin, Cout, s, F in PROD_LAYERS:
        assert any(c[:4] == (Cin, Cout, s, F) and c[4] in {_prod_in_T(T, F) for T in PROD_T} for c in CONV_GRID), (Cin, Cout, s, F)
    # the production tiles the sweep claims: layer 3 on 4x16 at stride 1, layer 4's downsampling conv on 2x32 at stride 2
    for T in (51, 101, 201, 301, 501):
        F3, T3 = RN.DEFAULT_RESNET.map_sizes(T)[3]
        assert pick_tile(F3, T3, 1) == (4, 16), T
    for T in (151, 201, 501):
        F4, T4 = RN.DEFAULT_RESNET.map_sizes(T)[4]
        assert pick_tile(F4, T4, 2) == (2, 32), T


# ------------------------------------------------------------------------------------------------------------------------------- GPU
def _dt(f16):
    return torch.float16 if f16 else torch.bfloat16


def _bits(f16):
    return 11 if f16 else 8


def _args(x, W, bias, y, B, F, T, Cin, Cout, stride, f16, relu=True, sc=None, Csc=0, Fsc=0, Tsc=0, sc_stride=0, res=None, ldx=0):
    """sdk_resnet_conv_args from device pointers (ints) or tensors."""
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    a = LIB.ResNetConvArgs()
    a.x, a.W, a.bias, a.y, a.sc, a.res, a.ldx = p(x), p(W), p(bias), p(y), p(sc), p(res), ldx
    a.B, a.F, a.T, a.Cin, a.Cout, a.stride = B, F, T, Cin, Cout, stride
    a.Csc, a.Fsc, a.Tsc, a.stride_sc = Csc, Fsc, Tsc, sc_stride
    a.flags = (LIB.GEMM_RELU if relu else 0) | (LIB.GEMM_F16 if f16 else 0)
    return a


def _conv(engine, x, wk, bias, B, F, T, Cin, Cout, stride, f16, **kw):
    """One sdk_resnet_conv2d into a sentinel-filled buffer with a guard of one full tile behind y; the guard must come back untouched."""
    Fo, To = _out(F, stride), _out(T, stride)
    n, guard = B * Fo * To * Cout, 64 * Cout
    buf = torch.full((n + guard,), SENTINEL, dtype=_dt(f16), device="cuda")
    a = _args(x, wk, bias, buf, B, F, T, Cin, Cout, stride, f16, **kw)
    LIB.check(engine.lib.sdk_resnet_conv2d(engine.ctx, C.byref(a), None), "sdk_resnet_conv2d")
    torch.cuda.synchronize()
    buf = buf.cpu()
    assert bool((buf[n:] == SENTINEL).all()), "sdk_resnet_conv2d wrote past y"
    return buf[:n].reshape(B, Fo, To, Cout)


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


@pytest.mark.gpu
@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CONV_GRID, ids=_case_id)
def test_conv2d_integer_exact_over_the_tiling_space(engine, case, f16):
    """Small-integer operands: the fp32 accumulation is exact and every |result| is an integer below 256 (bf16) / 2048 (fp16), so the GPU must
    equal the float64 conv rounded once, bit for bit, at every tile shape, kernel instance and edge map of CONV_GRID; B = 3, so segment
    boundaries cross tile rows.  Positions outside the map must not be stored (the guard behind y)."""
    Cin, Cout, s, F, T, relu = case
    g = torch.Generator().manual_seed(Cin * 7919 + Cout * 104729 + F * 131 + T + 17 * s + int(f16))
    B = 3
    lo, hi, lim = (-2, 2, 2048) if f16 else (-1, 1, 256)
    Fo, To = _out(F, s), _out(T, s)
    x = _ints(g, (B, F, T, Cin), lo, hi)
    wk = _ints(g, (Cout, 9 * Cin), lo, hi)
    bias = _ints(g, (Cout,), -4, 4)
    res = _ints(g, (B, Fo, To, Cout), -8, 8) if _has_res(Cin, Cout, s) else None
    want = RR.conv_ref(x, wk, bias, s, res=res, relu=relu)
    assert float(want.abs().max()) < lim, "operands too large for an exact rounded result"
    dt = _dt(f16)
    got = _conv(engine, x.to(dt).cuda(), wk.to(dt).cuda(), bias.float().cuda(), B, F, T, Cin, Cout, s, f16, relu=relu,
                res=res.to(dt).cuda() if res is not None else None)
    assert torch.equal(got, want.to(dt)), float((got.double() - want).abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("T,ldx", [(9, 80), (51, 88), (201, 96)])
def test_stem_integer_exact(engine, f16, relu, T, ldx):
    """The stem (Cin = 1) reading the fbank matrix [B*T, ldx]: padding columns hold a sentinel that would show if read; ReLU on and off."""
    g = torch.Generator().manual_seed(T * 10 + int(f16) * 2 + int(relu))
    B, F = 3, 80
    dt = _dt(f16)
    img = _ints(g, (B, T, F), -3, 3)
    feats = torch.full((B * T, ldx), 1000.0, dtype=dt)
    feats[:, :F] = img.reshape(B * T, F).to(dt)
    wk = _ints(g, (32, 9), -3, 3)
    bias = _ints(g, (32,), -4, 4)
    got = _conv(engine, feats.cuda(), wk.to(dt).cuda(), bias.float().cuda(), B, F, T, 1, 32, 1, f16, relu=relu, ldx=ldx)
    want = RR.conv_ref(img.transpose(1, 2).unsqueeze(-1), wk, bias, 1, relu=relu)
    assert float(want.abs().max()) < 256
    assert torch.equal(got, want.to(dt)), float((got.double() - want).abs().max())


def assert_storage_close(got, want, mag, K, bits, what, frac_exact=0.99):
    """got: the stored GPU result; want: float64 of the same stored operands (before the rounding).  Every element within half a storage ulp of
    want plus the fp32 accumulation allowance K 2^-24 mag (mag = |x| (*) |W| + |bias| + |res|, K = 9 Cin + Csc); >= frac_exact of the elements
    bit-identical to want rounded once.  -> (fraction bit-identical, worst |got - want| / bound)."""
    g = got.double().cpu()
    want, mag = want.cpu(), mag.cpu()
    tol = 0.5 * torch.maximum(RR.storage_ulp(g, bits), RR.storage_ulp(want, bits)) + K * U32 * mag
    err = (g - want).abs()
    bad = err > tol
    assert not bad.any(), (f"{what}: {int(bad.sum())} / {bad.numel()} elements outside half a storage ulp + K u |terms|; worst excess "
                           f"{float((err - tol).max()):.3e} at |want| {float(want.abs().flatten()[int((err - tol).argmax())]):.3e}")
    assert bool(torch.isfinite(g).all()), what
    same = float((g == RR.round_bits(want, bits)).double().mean())
    assert same >= frac_exact, f"{what}: only {same:.5f} of the elements bit-identical to the rounded float64 value"
    return same, float((err / tol.clamp_min(1e-300)).max())


# (name, Cin, Cout, stride, F, T, relu, kind): kind "res" = identity residual, "sc" = the downsampling conv2 with its projection shortcut
# (its input map [F][T] is the conv2's, the shortcut's [2F - 1][2T - 1] at stride 2), "" = neither
REAL_CASES = [
    ("layer1", 32, 32, 1, 80, 51, True, "res"),
    ("layer3_norelu", 128, 128, 1, 20, 51, False, "res"),
    ("layer4_conv1", 128, 256, 2, 20, 51, True, ""),
    ("layer2_conv2_sc", 64, 64, 1, 40, 26, True, "sc"),
    ("layer4_conv2_sc_norelu", 256, 256, 1, 10, 26, False, "sc"),
]


def _real_operands(g, Cin, Cout, s, F, T, kind, dt, scale=1.0, wscale=1.0, rscale=1.0):
    B = 3
    Fo, To = _out(F, s), _out(T, s)
    q = lambda t: t.to(dt).double()                                        # the stored operands
    x = q(torch.randn(B, F, T, Cin, generator=g, dtype=torch.float64) * scale)
    wk = q(torch.randn(Cout, 9 * Cin, generator=g, dtype=torch.float64) * math.sqrt(2.0 / (9 * Cin)) * wscale)
    bias = (torch.randn(Cout, generator=g, dtype=torch.float64) * 0.5).float().double()
    sc = wsc = res = None
    if kind == "res":
        res = q(torch.randn(B, Fo, To, Cout, generator=g, dtype=torch.float64) * rscale)
    elif kind == "sc":
        Csc = Cout // 2
        sc = q(torch.randn(B, 2 * F - 1, 2 * T - 1, Csc, generator=g, dtype=torch.float64) * scale)
        wsc = q(torch.randn(Cout, Csc, generator=g, dtype=torch.float64) * math.sqrt(2.0 / Csc) * wscale)
    return B, x, wk, bias, sc, wsc, res


def _run_real(engine, f16, Cin, Cout, s, F, T, relu, B, x, wk, bias, sc, wsc, res):
    dt = _dt(f16)
    kw = dict(relu=relu)
    W = wk
    if sc is not None:
        W = torch.cat([wk, wsc], 1)
        kw.update(sc=sc.to(dt).cuda(), Csc=sc.shape[-1], Fsc=sc.shape[1], Tsc=sc.shape[2], sc_stride=2)
    if res is not None:
        kw.update(res=res.to(dt).cuda())
    got = _conv(engine, x.to(dt).cuda(), W.to(dt).contiguous().cuda(), bias.float().cuda(), B, F, T, Cin, Cout, s, f16, **kw)
    want = RR.conv_ref(x, wk, bias, s, sc=sc, wsc=wsc, sc_stride=2, res=res, relu=relu)
    a = lambda t: None if t is None else t.abs()
    mag = RR.conv_ref(x.abs(), wk.abs(), bias.abs(), s, sc=a(sc), wsc=a(wsc), sc_stride=2, res=a(res), relu=False)
    K = 9 * Cin + (0 if sc is None else sc.shape[-1])
    return got, want, mag, K


@pytest.mark.gpu
@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", REAL_CASES, ids=[c[0] for c in REAL_CASES])
def test_conv2d_real_valued_against_float64(engine, case, f16):
    """Random operands at layer scale (x ~ N(0, 1), W ~ N(0, 2 / K), bias ~ N(0, 0.25), residual ~ N(0, 1)) in the storage format, against
    float64 of the same stored operands: every element within half a storage ulp + K 2^-24 (|x| (*) |W| + |bias| + |res|), and >= 99 % of the
    elements bit-identical to the float64 value rounded once.  Observed on an MI355X: bit-identical fractions 0.99981 .. 0.99996 in bf16 and
    0.99873 .. 0.99967 in fp16; the worst element reaches 0.98 of its bound in bf16, 0.89 in fp16."""
    name, Cin, Cout, s, F, T, relu, kind = case
    g = torch.Generator().manual_seed(Cin * 31 + T + int(f16))
    B, x, wk, bias, sc, wsc, res = _real_operands(g, Cin, Cout, s, F, T, kind, _dt(f16))
    got, want, mag, K = _run_real(engine, f16, Cin, Cout, s, F, T, relu, B, x, wk, bias, sc, wsc, res)
    same, worst = assert_storage_close(got, want, mag, K, _bits(f16), name)
    print(f"\n{name} {'fp16' if f16 else 'bf16'}: bit-identical {same:.6f}, worst |d| / bound {worst:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["res", ""])
def test_conv2d_fp16_saturates_at_65504(engine, kind):
    """fp16 storage: outputs beyond the finite range come back as +-65504 (never inf), equal to the saturated rounding RR.round_bits(., 11);
    the in-range ones keep the real-valued bound.  The identity residual read carries values up to ~6e4 in."""
    g = torch.Generator().manual_seed(65504 + len(kind))
    Cin = Cout = 64
    B, x, wk, bias, sc, wsc, res = _real_operands(g, Cin, Cout, 1, 10, 26, kind, torch.float16, scale=64.0, wscale=1000.0, rscale=20000.0)
    got, want, mag, K = _run_real(engine, True, Cin, Cout, 1, 10, 26, False, B, x, wk, bias, sc, wsc, res)
    g64 = got.double()
    assert bool(torch.isfinite(g64).all())
    sat = want.abs() >= 65520.0                                            # beyond the last fp16 rounding interval: inf in IEEE, 65504 here
    assert 0.2 < float(sat.double().mean()) < 0.9, float(sat.double().mean())
    assert bool((g64[sat].abs() == 65504.0).all()) and torch.equal(g64[sat], RR.round_bits(want[sat], 11))
    assert bool(((g64 > 0) == (want > 0))[sat].all())
    assert_storage_close(got[~sat], want[~sat], mag[~sat], K, 11, "fp16 in range")


# ---------------------------------------------------------------------------------------------------------- per-layer replay of the forward
def _slot(blob_cpu, off, n, dtype):
    return torch.from_numpy(blob_cpu[off:off + n * np.dtype(dtype).itemsize].view(dtype).copy())


def _replay(engine, rn, feats, ldf, B, T):
    """The conv sequence of sdk_resnet_forward (csrc/sdk_api.hip), one sdk_resnet_conv2d per conv on the blob's weight and bias slots, every
    output kept.  -> list of (name, inputs for RR.conv_ref, stored output [B, Fo, To, Cout] on the device)."""
    d, f16 = rn.desc, rn.precision == 2
    dt = _dt(f16)
    base = rn.blob.data_ptr()
    blob = rn.blob.cpu().numpy()

    def weights(i, cout, k):
        wk = _slot(blob, d.off[2 * i], cout * k, np.int16).view(dt).reshape(cout, k).double()
        return wk, _slot(blob, d.off[2 * i + 1], cout, np.float32).double()

    def launch(i, x, B_, F, Tl, Cin, Cout, s, ldx=0, sc=None, Csc=0, Fsc=0, Tsc=0, res=None):
        y = torch.full((B_, _out(F, s), _out(Tl, s), Cout), SENTINEL, dtype=dt, device="cuda")
        a = _args(x, base + d.off[2 * i], base + d.off[2 * i + 1], y, B_, F, Tl, Cin, Cout, s, f16, sc=sc, Csc=Csc, Fsc=Fsc, Tsc=Tsc,
                  sc_stride=2 if sc is not None else 0, res=res, ldx=ldx)
        LIB.check(engine.lib.sdk_resnet_conv2d(engine.ctx, C.byref(a), None), f"replayed conv {i}")
        return y

    out = []
    nf, C0 = d.n_feats, d.width[0]
    X = launch(0, feats, B, nf, T, 1, C0, 1, ldx=ldf)
    img = feats[:, :nf].reshape(B, T, nf).transpose(1, 2).unsqueeze(-1)      # the stem's image [B, F, T, 1]
    wk, bias = weights(0, C0, 9)
    out.append(("stem", dict(x=img, wk=wk, bias=bias, stride=1), X))
    F, Tl, Cc, conv = nf, T, C0, 1
    for l in range(4):
        for j in range(d.blocks[l]):
            s, Cw = (2 if (j == 0 and l > 0) else 1), d.width[l]
            proj = j == 0 and (s != 1 or Cc != Cw)
            H = launch(conv, X, B, F, Tl, Cc, Cw, s)
            wk, bias = weights(conv, Cw, 9 * Cc)
            out.append((f"layer{l + 1}.{j}.conv1", dict(x=X, wk=wk, bias=bias, stride=s), H))
            Fo, To = _out(F, s), _out(Tl, s)
            if proj:
                Y = launch(conv + 1, H, B, Fo, To, Cw, Cw, 1, sc=X, Csc=Cc, Fsc=F, Tsc=Tl)
                wk, bias = weights(conv + 1, Cw, 9 * Cw + Cc)
                ref = dict(x=H, wk=wk[:, :9 * Cw], bias=bias, stride=1, sc=X, wsc=wk[:, 9 * Cw:], sc_stride=s)
            else:
                Y = launch(conv + 1, H, B, Fo, To, Cw, Cw, 1, res=X)
                wk, bias = weights(conv + 1, Cw, 9 * Cw)
                ref = dict(x=H, wk=wk, bias=bias, stride=1, res=X)
            out.append((f"layer{l + 1}.{j}.conv2", ref, Y))
            X, F, Tl, Cc, conv = Y, Fo, To, Cw, conv + 2
    torch.cuda.synchronize()
    return out


def _embedding_bound(x, W, b, stats):
    """Bound on |fp32 embedding - float64 embedding| from the fp32 operation counts, per element [B, E].  x: the last map (>= 0, post-ReLU)
    [B, F4, T4, C]; W [E, 2 C F4]; b [E]; stats: float64 statistics [B, 2 C F4].
    A sum of n fp32 roundings is taken at lam sqrt(n) u (sum of |terms|), lam = 6: the probabilistic rounding-error bound (Higham and Mary,
    SIAM J. Sci. Comput. 41(5), 2019), which holds with probability >= 1 - 2 n exp(-lam^2 / 2) per sum (the worst case n u is ~ sqrt(n) times
    looser and, at n = 5120, above the 2.5e-4 max|want| this check must stay within).
      mean = fl(sum_t x) / T: T - 1 additions of nonnegative terms, the product by fl(1 / T): |d mean| <= lam sqrt(T + 1) u mean.
      var: q = sum_t (x - mean)^2 as T fmas on d = fl(x - mean) (2 u q from the rounding of d), the error of mean adds T d_mean^2 exactly;
           v = q fl(1 / (T - 1)) + 1e-7 (3 roundings): |d v| <= (lam sqrt(T) + 2) u q / (T - 1) + T d_mean^2 / (T - 1) + 3 u v.
      std = sqrt(v): |d std| <= |d v| / (2 std) + u std.
      seg_1: emb = W stats + b, the 5120-long dot products split into 16 K-slices of 320 fmas plus a 16-term sum and the bias (sdk_rows_fc):
           |d emb| <= sum_j |W_j| |d stats_j| + lam sqrt(320 + 16 + 1) u (sum_j |W_j stats_j| + |b|)."""
    lam = 6.0
    B, F4, T4, Cn = x.shape
    xs = x.double().permute(0, 3, 1, 2).reshape(B, -1, T4)
    mean = xs.mean(-1)
    q = ((xs - mean[..., None]) ** 2).sum(-1)
    std = stats[:, stats.shape[1] // 2:]
    dmean = lam * math.sqrt(T4 + 1) * U32 * mean
    dv = (lam * math.sqrt(T4) + 2) * U32 * q / (T4 - 1) + T4 * dmean ** 2 / (T4 - 1) + 3 * U32 * std ** 2
    dstd = dv / (2 * std) + U32 * std
    dstats = torch.cat([dmean, dstd], 1)
    n_fc = W.shape[1] // 16 + 16 + 1
    return dstats @ W.abs().T + lam * math.sqrt(n_fc) * U32 * (stats.abs() @ W.abs().T + b.abs())


REPLAY = [(0, 9, 2, 80), (0, 51, 2, 96), (0, 151, 2, 80), (0, 201, 1, 96), (0, 501, 1, 96),
          (2, 9, 2, 96), (2, 51, 2, 80), (2, 151, 2, 96), (2, 201, 1, 80), (2, 501, 1, 96)]


@pytest.mark.gpu
@pytest.mark.parametrize("precision,T,B,ldf", REPLAY, ids=[f"p{p}-T{T}-B{B}-ldf{l}" for p, T, B, l in REPLAY])
def test_resnet_forward_replayed_layer_by_layer(engine, precision, T, B, ldf):
    """The forward's 33 convs replayed through sdk_resnet_conv2d at production shapes (every layer's tile, both formats, the stem's feature
    stride at ldf = 80 and 96).  Each conv against float64 of its OWN stored inputs - no error carries across layers, so the per-layer bound of
    test_conv2d_real_valued_against_float64 applies to every layer.  Then sdk_resnet_forward on the same features against the float64 pooling of
    the replayed last map times seg_1, within _embedding_bound (asserted >= 100x tighter than the model-level test's 2.5e-2 max|want|): a slip
    in the pooling kernel, the forward's buffer rotation or shortcut / residual wiring, or seg_1 shows here.  Observed on an MI355X: every layer
    >= 0.99983 (bf16) / >= 0.99873 (fp16) bit-identical to its float64 value rounded once; embedding deviations 0.3 .. 0.6 % of the bound,
    which is 0.9e-4 .. 1.4e-4 max|want|."""
    f16 = precision == 2
    dt, bits = _dt(f16), _bits(f16)
    w = RN.synthetic_weights(0)
    rn = RN.ResNet34(engine, w, precision=precision)
    g = torch.Generator().manual_seed(T * 3 + precision)
    feats = torch.full((B * T, ldf), 5.0, dtype=dt)                          # the padding columns must never be read as data
    feats[:, :80] = (torch.randn(B * T, 80, generator=g) * 3.0).to(dt)
    feats = feats.cuda()
    convs = _replay(engine, rn, feats, ldf, B, T)
    assert len(convs) == 33
    worst, fracs = 0.0, []
    for name, ref, y in convs:
        inp = {k: (v.cpu().double() if torch.is_tensor(v) else v) for k, v in ref.items()}
        want = RR.conv_ref(inp["x"], inp["wk"], inp["bias"], inp["stride"], sc=inp.get("sc"), wsc=inp.get("wsc"),
                           sc_stride=inp.get("sc_stride", 1), res=inp.get("res"))
        a = lambda t: None if t is None else t.abs()
        mag = RR.conv_ref(inp["x"].abs(), inp["wk"].abs(), inp["bias"].abs(), inp["stride"], sc=a(inp.get("sc")), wsc=a(inp.get("wsc")),
                          sc_stride=inp.get("sc_stride", 1), res=a(inp.get("res")), relu=False)
        K = inp["wk"].shape[1] + (0 if inp.get("wsc") is None else inp["wsc"].shape[1])
        same, r = assert_storage_close(y.cpu(), want, mag, K, bits, f"{name} (p{precision} T={T})")
        worst, fracs = max(worst, r), fracs + [same]
    emb = rn.forward(feats, B, T)
    torch.cuda.synchronize()
    emb = emb.cpu().double()
    last = convs[-1][2].cpu().double()
    stats = RR.tstp_stats(last)
    W1, b1 = torch.from_numpy(w["seg_1.weight"]).double(), torch.from_numpy(w["seg_1.bias"]).double()
    want = stats @ W1.T + b1
    bound = _embedding_bound(last, W1, b1, stats)
    dev = (emb - want).abs()
    scale = float(want.abs().max())
    print(f"\nreplay p{precision} T={T} B={B}: per-layer worst |d| / bound {worst:.3f}, min bit-identical {min(fracs):.5f}; embedding max |d| "
          f"{float(dev.max()):.3e} = {float((dev / bound).max()):.3f} of its bound (bound max {float(bound.max()):.3e} = "
          f"{float(bound.max()) / scale:.2e} max|want|)")
    assert float(bound.max()) <= 2.5e-4 * scale, "the embedding bound must be >= 100x tighter than the model-level test's"
    assert bool((dev <= bound).all()), f"embedding off by {float(dev.max()):.3e} (bound {float(bound.max()):.3e})"


# ---------------------------------------------------------------------------------------------------------- large batch
@pytest.mark.gpu
def test_resnet_forward_at_the_default_batch_of_5s_windows(engine):
    """The Backend's default batch (SDK_MAX_BATCH = 2048) of 5-s windows (T = 501): the stem writes B F T = 82.1 M positions, more than the
    2^31 / 32 it used to accept (1674 segments here) and well under its int32 grid's 2^31 - 256.  The forward must run, and rows on both sides of
    1674 segments must equal B = 1 forwards of the same features bit for bit.  The 16 GB workspace is the test's own."""
    rn = RN.ResNet34(engine, RN.synthetic_weights(0))
    B, T, ldf = 2048, 501, 96
    gen = torch.Generator(device="cuda").manual_seed(2048)
    feats = torch.zeros(B * T, ldf, dtype=torch.bfloat16, device="cuda")
    feats[:, :80] = (torch.randn(B * T, 80, generator=gen, device="cuda") * 3.0).to(torch.bfloat16)
    lib = engine.lib
    ws = torch.empty(lib.sdk_resnet_workspace_bytes(C.byref(rn.desc), B, T), dtype=torch.uint8, device="cuda")
    emb = torch.full((B, 192), float("nan"), dtype=torch.float32, device="cuda")
    try:
        LIB.check(lib.sdk_resnet_forward(engine.ctx, rn.blob.data_ptr(), C.byref(rn.desc), feats.data_ptr(), ldf, B, T, ws.data_ptr(), ws.numel(),
                                         emb.data_ptr(), None), "sdk_resnet_forward")
        torch.cuda.synchronize()
    finally:
        del ws
        torch.cuda.empty_cache()
    assert bool(torch.isfinite(emb).all())
    for i in (0, 1673, 1674, 2047):
        e1 = rn.forward(feats[i * T:(i + 1) * T], 1, T)
        torch.cuda.synchronize()
        assert torch.equal(e1[0], emb[i]), i


# ---------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.gpu
def test_resnet_refusals_name_the_value_and_launch_nothing(engine):
    """Arguments sdk_resnet_conv2d / sdk_resnet_forward cannot serve: non-zero return, sdk_last_error() names the function and the value, the
    output stays untouched, and the context keeps working."""
    lib = engine.lib
    dev = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")
    x32, x48 = dev(1, 4, 4, 32), dev(1, 4, 4, 48)
    W = dev(256, 9 * 256 + 256)
    bias = torch.zeros(256, dtype=torch.float32, device="cuda")
    y = torch.full((2 * 4 * 4 * 256 + 64,), SENTINEL, dtype=torch.bfloat16, device="cuda")

    def refused(a, *pats):
        rc = lib.sdk_resnet_conv2d(engine.ctx, C.byref(a), None)
        msg = lib.sdk_last_error().decode()
        assert rc != 0 and "sdk_resnet_conv2d" in msg, (rc, msg)
        for p in pats:
            assert p in msg, (p, msg)

    refused(_args(x48, W, bias, y, 1, 4, 4, 48, 32, 1, False), "Cin=48")
    refused(_args(x32, W, bias, y, 1, 4, 4, 32, 32, 3, False), "stride=3")
    res, sc = dev(1, 4, 4, 32), dev(1, 7, 7, 32)
    refused(_args(x32, W, bias, y, 1, 4, 4, 32, 32, 1, False, sc=sc, Csc=32, Fsc=7, Tsc=7, sc_stride=2, res=res), "exclude each other")
    refused(_args(x32, W, bias, y, 1, 4, 4, 32, 32, 1, False, sc=dev(1, 9, 9, 32), Csc=32, Fsc=9, Tsc=9, sc_stride=2),
            "shortcut input [9][9][32] at stride 2", "4 x 4 output")
    refused(_args(x32, W, bias, y.data_ptr() + 2, 1, 4, 4, 32, 32, 1, False), "16-byte aligned", f"y={y.data_ptr() + 2:#x}")
    feats = dev(2 * 9, 96)
    refused(_args(feats, W, bias, y, 2, 80, 9, 1, 32, 2, False, ldx=96), "stem", "stride=2")
    refused(_args(feats, W, bias, y, 2, 80, 9, 1, 32, 1, False, ldx=64), "stem", "ldx=64")
    torch.cuda.synchronize()
    assert bool((y.cpu() == SENTINEL).all()), "a refused call launched"

    rn = RN.ResNet34(engine, RN.synthetic_weights(0))
    ws = torch.empty(lib.sdk_resnet_workspace_bytes(C.byref(rn.desc), 1, 51), dtype=torch.uint8, device="cuda")
    emb = torch.full((1, 192), SENTINEL, dtype=torch.float32, device="cuda")
    f = dev(51, 96)
    for T, ldf, pat in ((8, 96, "T=8"), (51, 64, "ldf=64")):
        rc = lib.sdk_resnet_forward(engine.ctx, rn.blob.data_ptr(), C.byref(rn.desc), f.data_ptr(), ldf, 1, T, ws.data_ptr(), ws.numel(),
                                    emb.data_ptr(), None)
        msg = lib.sdk_last_error().decode()
        assert rc != 0 and "sdk_resnet_forward" in msg and pat in msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool((emb.cpu() == SENTINEL).all())

    # the context is intact: a valid conv right after the refusals is exact
    g = torch.Generator().manual_seed(5)
    xi, wi, bi = _ints(g, (2, 4, 4, 32), -1, 1), _ints(g, (32, 288), -1, 1), _ints(g, (32,), -4, 4)
    got = _conv(engine, xi.to(torch.bfloat16).cuda(), wi.to(torch.bfloat16).cuda(), bi.float().cuda(), 2, 4, 4, 32, 32, 1, False)
    assert torch.equal(got, RR.conv_ref(xi, wi, bi, 1).to(torch.bfloat16))
