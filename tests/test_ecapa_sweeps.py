"""Kernel-level sweeps of the per-utterance ECAPA-TDNN kernels (csrc/pool_se.hip: SE, ASP statistics, ASP pooling, fused ASP) and of the
fused Res2Net chain (csrc/res2net.hip), in both 2-byte formats (fmt 0 = bf16, 2 = fp16: the _fmt entry points' `precision`), against the
float64 restatements of tests/sweeps_ref.py on the same stored inputs.  Shapes sit on the kernels' tile edges and dispatch boundaries;
the data include subnormal fp16 magnitudes, saturation, exact ties, one dominant frame, a transient frame 0 and NaN.  Every bound is
n 2^-24 sum|terms| (plus one storage ulp where the kernel stores); each case prints its worst error / bound."""
import ctypes as C

import pytest
import torch

import sweeps_ref as R
from conftest import sub
from oracle import ecapa as oecapa

pytestmark = pytest.mark.gpu

L = sub("_lib")
W = sub("weights")
WP = sub("weights_pack")
SdkError = L.SdkError
FMTS = [0, 2]
SENT = -7.75            # sentinel written around every output (exact in both formats)


def _s():
    return torch.cuda.current_stream().cuda_stream


def _dev(x, fmt):
    return x.to(R.FMTS[fmt]).cuda()


def judge(got, want, bound, what):
    """|got - want| <= bound elementwise (a NaN anywhere fails); prints and returns the worst error / bound"""
    got = got.double().cpu()
    err = (got - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} / {bad.numel()} outside the bound, worst err / bound {ratio:.3g}"
    print(f"{what}: worst err / bound {ratio:.3f}")
    return ratio


def judge_stored(got, want, acc, fmt, what, frac_exact):
    tgt, bound = R.stored_bound(want, acc, fmt)
    judge(got, tgt, bound, what)
    same = float((got.double().cpu() == R.store(want, fmt)).double().mean())
    assert same >= frac_exact, f"{what}: only {same:.4f} bit-identical to the rounded reference"


def _wide(rows, cols, extra_rows, extra_cols, fmt):
    """an output view [rows, cols] of a sentinel-filled [rows + extra_rows, cols + extra_cols] buffer"""
    buf = torch.full((rows + extra_rows, cols + extra_cols), SENT, dtype=R.FMTS[fmt], device="cuda")
    return buf, buf[:rows, :cols]


def _untouched(buf, rows, cols):
    b = buf.double().cpu()
    assert (b[:, cols:] == SENT).all() and (b[rows:, :] == SENT).all(), "store outside the output"


# ---------------------------------------------------------------------------------------------------- SE
def _se_call(eng, z, x, w1t, b1, w2t, b2, out, B, T, fmt, split, mean_in=None):
    C_, Cse = z.shape[1], w1t.shape[1]
    ws = torch.empty(eng.lib.sdk_se_workspace_bytes(B, C_, Cse), dtype=torch.uint8, device="cuda") if split else None
    L.check(eng.lib.sdk_se_gate_residual_fmt(eng.ctx, z.data_ptr(), z.stride(0), x.data_ptr(), x.stride(0), w1t.data_ptr(), b1.data_ptr(),
                                             w2t.data_ptr(), b2.data_ptr(), out.data_ptr(), out.stride(0), B, T, C_, Cse,
                                             mean_in.data_ptr() if mean_in is not None else None, ws.data_ptr() if split else None,
                                             ws.numel() if split else 0, fmt, _s()), "sdk_se_gate_residual_fmt")


def _se_data(B, T, C, Cse, fmt, seed, mag=1.0):
    g = torch.Generator().manual_seed(seed)
    z = R.store(torch.randn(B * T, C, generator=g) * 2 * mag, fmt)
    x = R.store(torch.randn(B * T, C, generator=g) * mag, fmt)
    if fmt == 2 and mag == 1.0 and T > 2:                          # saturation: g z + x past 65504 in a few elements
        z[T // 2, :4] = 60000.0
        x[T // 2, :4] = 60000.0
    w1t = torch.randn(C, Cse, generator=g) / C ** 0.5
    w2t = torch.randn(Cse, C, generator=g) * 2 / Cse ** 0.5
    b1, b2 = torch.randn(Cse, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    return z, x, w1t, b1, w2t, b2


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("C,Cse", [(C_, Cse_) for C_ in (64, 256, 1024, 2048) for Cse_ in (32, 64, 128, 256) if Cse_ <= C_])
def test_se_sweep(engine, fmt, C, Cse):
    """both schedules (split with workspace, one kernel per segment) and the split form with a given mean; strided z / x / out; T on
    the SE_TCH = 32 tiles, the 4-way unrolled stripe tail and ngrp = 1 (C = 2048); fp16 subnormals at T = 33"""
    B = 3
    for T in (1, 2, 3, 31, 32, 33, 201, 501):
        mag = 1e-5 if T == 33 else 1.0
        z, x, w1t, b1, w2t, b2 = _se_data(B, T, C, Cse, fmt, C + T, mag)
        zw = _dev(torch.cat([z, torch.full((B * T, 8), 3.0)], 1), fmt)[:, :C]
        xw = _dev(torch.cat([x, torch.full((B * T, 16), 3.0)], 1), fmt)[:, :C]
        want, acc = R.se_ref(z, x, w1t, b1, w2t, b2, B, T)
        dw = [t.cuda() for t in (w1t, b1, w2t, b2)]
        mean = z.reshape(B, T, C).mean(1).float().cuda()
        for split, mean_in in ((True, None), (False, None), (True, mean)):
            buf, out = _wide(B * T, C, 5, 24, fmt)
            _se_call(engine, zw, xw, *dw, out, B, T, fmt, split, mean_in)
            torch.cuda.synchronize()
            _untouched(buf, B * T, C)
            judge_stored(out, want, acc, fmt, f"se fmt {fmt} C {C} Cse {Cse} T {T} split {split} mean_in {mean_in is not None}", 0.97)


def test_se_refusals(engine):
    z = torch.zeros(2 * 8, 768, dtype=torch.bfloat16, device="cuda")
    w1t, b1, w2t, b2 = torch.zeros(768, 64).cuda(), torch.zeros(64).cuda(), torch.zeros(64, 768).cuda(), torch.zeros(768).cuda()
    with pytest.raises(SdkError, match="C=768 unsupported"):
        _se_call(engine, z, z, w1t, b1, w2t, b2, torch.empty_like(z), 2, 8, 0, True)
    z = z[:, :256].contiguous()
    with pytest.raises(SdkError, match="precision=1"):
        _se_call(engine, z, z, w1t[:256], b1, w2t[:, :256].contiguous(), b2[:256], torch.empty_like(z), 2, 8, 1, True)


# ---------------------------------------------------------------------------------------------------- ASP statistics / pooling
def _stats_call(eng, h, B, T, fmt):
    Cm = h.shape[1]
    out = torch.empty((B, 2 * Cm), dtype=torch.float32, device="cuda")
    L.check(eng.lib.sdk_asp_stats_fmt(eng.ctx, h.data_ptr(), h.stride(0), B, T, Cm, out.data_ptr(), fmt, _s()), "sdk_asp_stats_fmt")
    return out


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("C", [8, 1000, 1032, 3072])
def test_asp_stats_sweep(engine, fmt, C):
    """tails of the 1024-channel grid, ldh > C; channels 0..7 at a large mean with a small spread (1000 + N(0, 1): the bound follows the
    terms about h[t = 0] - small here - not the mean); fp16 subnormals at T = 3"""
    B = 2
    for T in (1, 2, 3, 201, 3001):
        g = torch.Generator().manual_seed(C + T)
        h = torch.randn(B * T, C, generator=g) * (1e-5 if T == 3 else 3) + (0 if T == 3 else 1)
        h[:, :8] = 1000 + torch.randn(B * T, 8, generator=g)
        h = R.store(h, fmt)
        hw = _dev(torch.cat([h, torch.zeros(B * T, 8)], 1), fmt)[:, :C]
        got = _stats_call(engine, hw, B, T, fmt)
        want, bound = R.asp_stats_ref(h, B, T)
        torch.cuda.synchronize()
        judge(got, want, bound, f"asp_stats fmt {fmt} C {C} T {T}")


def _pool_call(eng, logits, h, B, T, fmt):
    Cm = h.shape[1]
    out = torch.empty((B, 2 * Cm), dtype=torch.float32, device="cuda")
    L.check(eng.lib.sdk_asp_pool_fmt(eng.ctx, logits.data_ptr(), logits.stride(0), h.data_ptr(), h.stride(0), B, T, Cm, out.data_ptr(), fmt, _s()),
            "sdk_asp_pool_fmt")
    return out


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("C", [64, 192, 3072])
def test_asp_pool_sweep(engine, fmt, C):
    """logits spread over +-80, exact ties (channels 0..7 constant over frames), one dominant frame (channels 8..15), fp16 subnormal h at T = 2"""
    B = 2
    for T in (1, 2, 225, 501, 3001):
        g = torch.Generator().manual_seed(7 * C + T)
        lg = (torch.rand(B * T, C, generator=g) * 160 - 80)
        lg[:, :8] = 1.5
        lg[:, 8:16] = torch.randn(B * T, 8, generator=g)
        lg.view(B, T, C)[:, T // 3, 8:16] += 30
        h = R.store(torch.randn(B * T, C, generator=g) * (1e-5 if T == 2 else 2) + (0 if T == 2 else 3), fmt)
        got = _pool_call(engine, lg.cuda(), _dev(h, fmt), B, T, fmt)
        want, bound = R.asp_pool_ref(lg, h, B, T)
        torch.cuda.synchronize()
        judge(got, want, bound, f"asp_pool fmt {fmt} C {C} T {T}")


# ---------------------------------------------------------------------------------------------------- fused ASP
def _fused_call(eng, ah, w2, b2, h, B, T, fmt, kblocked=False):
    Cm = w2.shape[0]
    out = torch.empty((B, 2 * Cm), dtype=torch.float32, device="cuda")
    if kblocked:
        L.check(eng.lib.sdk_asp_fused_kblocked_fmt(eng.ctx, ah.data_ptr(), ah.stride(0), w2.data_ptr(), b2.data_ptr(), h.data_ptr(), B, T, Cm,
                                                   ah.shape[1], out.data_ptr(), fmt, _s()), "sdk_asp_fused_kblocked_fmt")
    else:
        L.check(eng.lib.sdk_asp_fused_fmt(eng.ctx, ah.data_ptr(), ah.stride(0), w2.data_ptr(), b2.data_ptr(), h.data_ptr(), h.stride(0), B, T, Cm,
                                          ah.shape[1], out.data_ptr(), fmt, _s()), "sdk_asp_fused_fmt")
    return out


def _fused_data(B, T, C, fmt, seed, mag=1.0):
    g = torch.Generator().manual_seed(seed)
    h = R.store(torch.randn(B * T, C, generator=g) * 3 * mag + 2 * mag, fmt)
    ah = R.store(torch.tanh(torch.randn(B * T, 128, generator=g)), fmt)
    w2 = R.store(torch.randn(C, 128, generator=g) * 0.3, fmt)
    b2 = torch.randn(C, generator=g)
    return h, ah, w2, b2


# (T, C, asp_per_segment): asp_fused_kernel<3> (T <= 96), <7> (C % 256 != 0, T > 208, or the option off), asp_seg_kernel (nblk 8 .. 96)
FUSED_CASES = [(1, 256, 1), (31, 384, 1), (32, 256, 1), (33, 256, 1), (96, 384, 1), (97, 384, 1), (150, 3072, 0), (209, 256, 1), (224, 384, 1),
               (97, 256, 1), (128, 768, 1), (160, 3072, 1), (192, 256, 1), (193, 768, 1), (207, 3072, 1), (208, 256, 1)]


@pytest.mark.parametrize("fmt", FMTS)
def test_asp_fused_sweep(engine, fmt):
    """every dispatch of sdk_asp_fused; where the per-segment kernel runs, the K-blocked h must give the same bits; fp16 subnormal h at T = 33"""
    for T, C, per_seg in FUSED_CASES:
        B = 2
        h, ah, w2, b2 = _fused_data(B, T, C, fmt, T * 3 + C, 1e-5 if T == 33 else 1.0)
        dh, dah, dw2 = _dev(h, fmt), _dev(ah, fmt), _dev(w2, fmt)
        engine.set_option("asp_per_segment", per_seg)
        try:
            got = _fused_call(engine, dah, dw2, b2.cuda(), dh, B, T, fmt)
            if engine.lib.sdk_asp_kblocked_ok(engine.ctx, T, C):
                kb = _fused_call(engine, dah, dw2, b2.cuda(), engine.to_kblocked(dh), B, T, fmt, kblocked=True)
                torch.cuda.synchronize()
                assert torch.equal(got, kb), f"K-blocked h differs at T {T} C {C}"
        finally:
            engine.set_option("asp_per_segment", 1)
        want, bound = R.asp_fused_ref(ah, w2, b2, h, B, T)
        torch.cuda.synchronize()
        judge(got, want, bound, f"asp_fused fmt {fmt} T {T} C {C} per_segment {per_seg}")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("T,per_seg", [(64, 1), (150, 1), (150, 0), (220, 1)])
def test_asp_fused_transient_frame0(engine, fmt, T, per_seg):
    """frame 0 sits 50 sigma off the attended frames and the attention peaks away from it: a single pass about h[t = 0] loses the
    variance's low bits to cancellation ((h0 - mu)^2 / var = 2500); the bound is the two-pass one"""
    B, C = 2, 256
    g = torch.Generator().manual_seed(T)
    h = torch.randn(B * T, C, generator=g)
    h.view(B, T, C)[:, 0] += 50
    h = R.store(h, fmt)
    ah = torch.randn(B * T, 128, generator=g) * 0.05
    ah[:, 0] = 0
    ah.view(B, T, 128)[:, T // 2:T // 2 + 10, 0] = 6.0
    ah = R.store(ah, fmt)
    w2 = torch.randn(C, 128, generator=g) * 0.1
    w2[:, 0] = 1.0
    w2 = R.store(w2, fmt)
    b2 = torch.zeros(C)
    engine.set_option("asp_per_segment", per_seg)
    try:
        got = _fused_call(engine, _dev(ah, fmt), _dev(w2, fmt), b2.cuda(), _dev(h, fmt), B, T, fmt)
    finally:
        engine.set_option("asp_per_segment", 1)
    want, bound = R.asp_fused_ref(ah, w2, b2, h, B, T)
    torch.cuda.synchronize()
    judge(got, want, bound, f"asp_fused transient frame 0 fmt {fmt} T {T} per_segment {per_seg}")


# ---------------------------------------------------------------------------------------------------- NaN
@pytest.mark.parametrize("fmt", FMTS)
def test_nan_propagates_to_the_outputs_that_read_it(engine, fmt):
    """a NaN in one frame of z (SE) or h (ASP) must come out as NaN where the kernel reads it directly.  SE: the output element is NaN
    (fp16 storage turned it into -65504 before the fix).  The rest of that segment is NOT NaN, by the kernels' ReLU semantics: the
    channel's mean is NaN, so every FC1 pre-activation is NaN, and the ReLU (fmaxf, as in every ReLU epilogue of the library) maps it to
    0 - the gate is sigmoid(b2) and the other outputs are fmt(sigmoid(b2) z + x), asserted below.  ASP: the channel's mean and std are
    NaN (the std floor max(var, 1e-12) turned a NaN variance into 1e-6 before the fix), every other channel is finite."""
    B, T, C, Cse = 2, 40, 256, 64
    z, x, w1t, b1, w2t, b2 = _se_data(B, T, C, Cse, fmt, 5)
    z[T + 3, 17] = float("nan")
    dz, dx = _dev(z, fmt), _dev(x, fmt)
    for split in (True, False):
        out = torch.empty_like(dz)
        _se_call(engine, dz, dx, w1t.cuda(), b1.cuda(), w2t.cuda(), b2.cuda(), out, B, T, fmt, split)
        o = out.double().cpu()
        assert torch.isnan(o[T + 3, 17]) and int(torch.isnan(o).sum()) == 1, f"split {split}: NaN count {int(torch.isnan(o).sum())}"
        gate = torch.sigmoid(b2.double())
        zs, xs = z[T:].clone(), x[T:]
        zs[3, 17] = 0.0
        want = gate * zs + xs
        acc = (b2.double().abs() + 8) * R.EPS32 * zs.abs() + 2 * R.EPS32 * ((gate * zs).abs() + xs.abs())
        keep = torch.ones_like(want, dtype=torch.bool)
        keep[3, 17] = False
        tgt, bound = R.stored_bound(want, acc, fmt)
        judge(o[T:][keep], tgt[keep], bound[keep], f"se NaN segment, gate sigmoid(b2), fmt {fmt} split {split}")
    h, ah, w2, b2 = _fused_data(B, 150, 256, fmt, 9)
    h[150 + 70, 33] = float("nan")
    for T_, per_seg in ((150, 1), (150, 0), (64, 1)):
        hh, aa = h[:2 * T_], ah[:2 * T_]
        if T_ != 150:
            hh = hh.clone()
            hh[T_ + 20, 33] = float("nan")
        engine.set_option("asp_per_segment", per_seg)
        try:
            p = _fused_call(engine, _dev(aa, fmt), _dev(w2, fmt), b2.cuda(), _dev(hh, fmt), 2, T_, fmt).cpu()
        finally:
            engine.set_option("asp_per_segment", 1)
        nan = torch.isnan(p)
        assert nan[1, 33] and nan[1, 256 + 33] and int(nan.sum()) == 2, (T_, per_seg, int(nan.sum()))
    st = _stats_call(engine, _dev(h, fmt), 2, 150, fmt).cpu()
    assert torch.isnan(st[1, 33]) and torch.isnan(st[1, 256 + 33]) and int(torch.isnan(st).sum()) == 2
    lg = torch.randn(300, 256)
    pl = _pool_call(engine, lg.cuda(), _dev(h, fmt), 2, 150, fmt).cpu()
    assert torch.isnan(pl[1, 33]) and torch.isnan(pl[1, 256 + 33]) and int(torch.isnan(pl).sum()) == 2
    # the GEMM's fused column statistics (SE squeeze / ASP context / x-vector pooling) keep a NaN row's NaN in the segment's mean and std
    M, Tg, N, Cin = 1608, 201, 512, 64
    assert engine.lib.sdk_conv_gemm_stats_fusable(M, N, Tg)
    gA = torch.Generator().manual_seed(4)
    A = torch.randn(M, Cin, generator=gA)
    A[3 * Tg + 10, 5] = float("nan")
    Wt = torch.randn(N, Cin, generator=gA) * 0.1
    st = _gemm_stats(engine, _dev(A, fmt), _dev(Wt, fmt), Tg, fmt).cpu()
    nan = torch.isnan(st)
    assert nan[3].all() and not nan[torch.arange(8) != 3].any(), int(nan.sum())


# ---------------------------------------------------------------------------------------------------- Engine wrappers
def test_engine_wrappers_take_the_format_from_the_dtype(engine):
    """the context option "precision" stays 0; fp16 tensors must be read as fp16 (they were read as bf16 before the _fmt entry points)"""
    B, T, C, Cse, fmt = 2, 120, 256, 64, 2
    z, x, w1t, b1, w2t, b2 = _se_data(B, T, C, Cse, fmt, 11)
    want, acc = R.se_ref(z, x, w1t, b1, w2t, b2, B, T)
    for split in (True, False):
        out = engine.se_gate_residual(_dev(z, fmt), _dev(x, fmt), w1t.cuda(), b1.cuda(), w2t.cuda(), b2.cuda(), B, T, split=split)
        torch.cuda.synchronize()
        assert out.dtype == torch.float16
        judge_stored(out, want, acc, fmt, f"Engine.se_gate_residual fp16 split {split}", 0.97)
    h, ah, w2, fb2 = _fused_data(B, T, C, fmt, 12)
    st = engine.asp_stats(_dev(h, fmt), B, T)
    want, bound = R.asp_stats_ref(h, B, T)
    judge(st, want, bound, "Engine.asp_stats fp16")
    lg = torch.randn(B * T, C) * 3
    pl = engine.asp_pool(lg.cuda(), _dev(h, fmt), B, T)
    want, bound = R.asp_pool_ref(lg, h, B, T)
    judge(pl, want, bound, "Engine.asp_pool fp16")
    pf = engine.asp_fused(_dev(ah, fmt), _dev(w2, fmt), fb2.cuda(), _dev(h, fmt), B, T)
    want, bound = R.asp_fused_ref(ah, w2, fb2, h, B, T)
    judge(pf, want, bound, "Engine.asp_fused fp16")
    pk = engine.asp_fused(_dev(ah, fmt), _dev(w2, fmt), fb2.cuda(), engine.to_kblocked(_dev(h, fmt)), B, T, kblocked=True)
    torch.cuda.synchronize()
    assert torch.equal(pf, pk)
    with pytest.raises(ValueError, match="bfloat16 or float16"):
        engine.asp_stats(h.float().cuda(), B, T)
    with pytest.raises(ValueError, match="share one element format"):
        engine.asp_fused(_dev(ah, 0), _dev(w2, fmt), fb2.cuda(), _dev(h, fmt), B, T)
    for name in ("sdk_asp_pool_fmt", "sdk_asp_fused_fmt", "sdk_res2net_chain_fmt"):
        assert hasattr(engine.lib, name)
    with pytest.raises(SdkError, match="precision=3"):
        _stats_call(engine, _dev(h, fmt), B, T, 3)
    with pytest.raises(SdkError, match="sdk_asp_pool_fmt: precision=1"):
        _pool_call(engine, lg.cuda(), _dev(h, fmt), B, T, 1)


# ---------------------------------------------------------------------------------------------------- Res2Net chain
def _ptrs(ts, ctype=C.c_void_p):
    return (ctype * 7)(*[t.data_ptr() for t in ts] + [ts[0].data_ptr()] * (7 - len(ts)))


def _chain_call(eng, U, R_, Ws, bs, ss, hs, nconv, B, T, dil, fmt):
    L.check(eng.lib.sdk_res2net_chain_fmt(eng.ctx, U.data_ptr(), U.stride(0), R_.data_ptr(), R_.stride(0), _ptrs(Ws), _ptrs(bs), _ptrs(ss),
                                          _ptrs(hs), nconv, B, T, dil, fmt, _s()), "sdk_res2net_chain_fmt")


def _chain_run(eng, U, Ws, bs, ss, hs, nconv, B, T, dil, fmt, inplace):
    """returns (R as float64 [B*T, ldr] including chunk 0 and the columns past the chain, the buffer's width actually used)"""
    width = 128 * (nconv + 1)
    dW = [_dev(w, fmt) for w in Ws]
    db, ds, dh = ([t.float().cuda() for t in ts] for ts in (bs, ss, hs))
    if inplace:
        buf = _dev(torch.cat([U, torch.full((U.shape[0], 64), SENT)], 1), fmt)
        _chain_call(eng, buf, buf, dW, db, ds, dh, nconv, B, T, dil, fmt)
    else:
        dU = _dev(torch.cat([U, torch.zeros(U.shape[0], 8)], 1), fmt)
        buf = torch.full((U.shape[0], width + 136), SENT, dtype=R.FMTS[fmt], device="cuda")
        _chain_call(eng, dU, buf, dW, db, ds, dh, nconv, B, T, dil, fmt)
    torch.cuda.synchronize()
    out = buf.double().cpu()
    if inplace:
        assert torch.equal(out[:, :128], R.store(U[:, :128], fmt)) and (out[:, width:] == SENT).all()
    else:
        assert (out[:, :128] == SENT).all() and (out[:, width:] == SENT).all()
    return out


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("nconv,dil", [(1, 2), (3, 3), (7, 4), (7, 2)])
def test_res2net_chain_integer_exact(engine, fmt, nconv, dil):
    """integer operands (sweeps_ref.integer_chain_case): the chain must equal the float64 chain bit for bit, in place and out of place,
    in the 8-wave (T <= 112 / two_per_cu off) and 4-wave two-per-CU (T > 112) kernels"""
    for T in sorted({dil + 1, 9, 16, 17, 112, 113, 200, 208}):
        for B in (1, 5):
            U, Ws, bs, ss, hs = R.integer_chain_case(B, T, nconv, fmt, seed=T * 8 + nconv + B)
            want = torch.cat(R.res2net_chain_ref(U, Ws, bs, ss, hs, nconv, T, dil, fmt, exact=True), 1)
            for inplace in (True, False):
                for two in ((1, 0) if T > 112 else (1,)):
                    engine.set_option("res2net_two_per_cu", two)
                    try:
                        out = _chain_run(engine, U, Ws, bs, ss, hs, nconv, B, T, dil, fmt, inplace)
                    finally:
                        engine.set_option("res2net_two_per_cu", 1)
                    assert torch.equal(out[:, 128:128 * (nconv + 1)], want), f"T {T} B {B} in place {inplace} two_per_cu {two}"


def _gemm(eng, A, Wt, T, dil, bias, scale, shift, fmt):
    """one chain conv as sdk_conv_gemm (taps 3, ReLU, bias / scale / shift epilogue; SDK_GEMM_F16 for fp16)"""
    M = A.shape[0]
    g = L.ConvGemmArgs()
    out = torch.empty((M, 128), dtype=R.FMTS[fmt], device="cuda")
    g.A, g.lda, g.W, g.C, g.ldc = A.data_ptr(), A.stride(0), Wt.data_ptr(), out.data_ptr(), 128
    g.bias, g.scale, g.shift = bias.data_ptr(), scale.data_ptr(), shift.data_ptr()
    g.M, g.N, g.Cin, g.taps, g.dil, g.T = M, 128, 128, 3, dil, T
    g.flags = L.GEMM_RELU | (L.GEMM_F16 if fmt == 2 else 0)
    L.check(eng.lib.sdk_conv_gemm(eng.ctx, C.byref(g), _s()), "sdk_conv_gemm")
    torch.cuda.synchronize()
    return out.double().cpu()


def _gemm_stats(eng, A, Wt, T, fmt):
    """a 1x1 sdk_conv_gemm (no epilogue) with fused mean | std column statistics per segment -> [M / T, 2 N] fp32"""
    M, N = A.shape[0], Wt.shape[0]
    g = L.ConvGemmArgs()
    out = torch.empty((M, N), dtype=R.FMTS[fmt], device="cuda")
    part = torch.empty(eng.lib.sdk_conv_gemm_stats_bytes(M, N, 2), dtype=torch.uint8, device="cuda")
    g.A, g.lda, g.W, g.C, g.ldc = A.data_ptr(), A.stride(0), Wt.data_ptr(), out.data_ptr(), N
    g.M, g.N, g.Cin, g.taps, g.dil, g.T = M, N, A.shape[1], 1, 1, T
    g.flags = L.GEMM_F16 if fmt == 2 else 0
    g.stats_mode, g.stats_part = 2, part.data_ptr()
    L.check(eng.lib.sdk_conv_gemm(eng.ctx, C.byref(g), _s()), "sdk_conv_gemm")
    st = torch.empty((M // T, 2 * N), dtype=torch.float32, device="cuda")
    L.check(eng.lib.sdk_colstats_finish(eng.ctx, part.data_ptr(), M, N, T, 2, st.data_ptr(), _s()), "sdk_colstats_finish")
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("T,dil", [(9, 4), (100, 2), (113, 3), (208, 4)])
def test_res2net_chain_real_operands(engine, fmt, T, dil):
    """random operands: every conv y_c against float64 of its own stored input fmt(u_c + y_{c-1}) (one storage ulp + the K = 384 fp32
    accumulation), and bit for bit against the same conv as an sdk_conv_gemm launch (the header's contract); fp16 subnormal u at T = 9"""
    B, nconv = 3, 7
    g = torch.Generator().manual_seed(T + fmt)
    mag = 1e-4 if T == 9 else 1.0
    U = R.store(torch.randn(B * T, 128 * 8, generator=g) * mag, fmt)
    Ws = [R.store(torch.randn(128, 384, generator=g) / 384 ** 0.5 * 1.5, fmt) for _ in range(nconv)]
    bs = [(torch.randn(128, generator=g) * 0.1 * mag).double() for _ in range(nconv)]
    ss = [(torch.rand(128, generator=g) + 0.5).double() for _ in range(nconv)]
    hs = [(torch.randn(128, generator=g) * 0.1 * mag).double() for _ in range(nconv)]
    out = _chain_run(engine, U, Ws, bs, ss, hs, nconv, B, T, dil, fmt, inplace=False)
    prev = None
    for c in range(1, nconv + 1):
        s = U[:, 128 * c:128 * (c + 1)] if c == 1 else R.chain_input(U[:, 128 * c:128 * (c + 1)], prev, fmt)
        y, acc = R.tdnn_ref(s, Ws[c - 1], bs[c - 1], ss[c - 1], hs[c - 1], T, dil)
        got = out[:, 128 * c:128 * (c + 1)]
        judge_stored(got, y, acc, fmt, f"res2net conv {c} fmt {fmt} T {T} dil {dil}", 0.98)
        gm = _gemm(engine, _dev(s, fmt), _dev(Ws[c - 1], fmt), T, dil, bs[c - 1].float().cuda(), ss[c - 1].float().cuda(), hs[c - 1].float().cuda(), fmt)
        assert torch.equal(gm, got), f"conv {c}: chain and sdk_conv_gemm differ"
        prev = got


def test_res2net_chain_fmt_refusal(engine):
    U = torch.zeros(20, 1024, dtype=torch.float16, device="cuda")
    w = [torch.zeros(128, 384, dtype=torch.float16, device="cuda")]
    v = [torch.zeros(128, device="cuda")]
    with pytest.raises(SdkError, match="sdk_res2net_chain_fmt: precision=1"):
        _chain_call(engine, U, U, w, v, v, v, 1, 2, 10, 2, 1)


# ---------------------------------------------------------------------------------------------------- the fp16 forward
def _feats16(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(B, T, 80, generator=g) * 3.0
    f = torch.zeros(B * T, WP.N_MELS_PADDED, dtype=torch.float16)
    f[:, :80] = feats.reshape(-1, 80).to(torch.float16)
    return feats, f.cuda()


@pytest.fixture(scope="module")
def fp16_engine(engine):
    eng = sub("ops").Engine(0, bias_correction=False)
    eng.set_precision(2)
    yield eng
    eng.set_precision(0)


@pytest.mark.parametrize("B,T", [(3, 9), (3, 100), (2, 113), (3, 201), (2, 208)])
def test_fp16_forward_switches_are_result_neutral(fp16_engine, B, T):
    """the fp16 twin of test_res2net_chain_fusion_is_bit_identical, with h_kblocked: every switch must leave the fp16 embedding's bits alone"""
    eng = fp16_engine
    _, f = _feats16(B, T, 31 + T)
    ref = eng.ecapa_forward(f, B, T).cpu()
    for name in ("res2net_chain_fusion", "res2net_packed_weights", "res2net_two_per_cu", "asp_packed_weights", "h_kblocked"):
        try:
            eng.set_option(name, 0)
            other = eng.ecapa_forward(f, B, T).cpu()
        finally:
            eng.set_option(name, 1)
        assert torch.equal(ref, other), f"{name} 0 changes the fp16 forward at T {T}: {float((ref - other).abs().max())}"


@pytest.mark.parametrize("B,T", [(2, 301), (1, 501)])
def test_fp16_forward_long_windows(fp16_engine, B, T):
    """T > 208 (unfused Res2Net chain) and T > 224 (fp32 logits + asp_pool<true>) in fp16 against the 11-bit oracle at
    test_gpu_fp16's tolerances"""
    eng = fp16_engine
    feats, f = _feats16(B, T, 23 + T)
    assert T > eng.lib.sdk_res2net_chain_max_frames() and T > eng.lib.sdk_asp_fused_max_frames()
    emb = eng.ecapa_forward(f, B, T).cpu()
    want = oecapa.EcapaOracle(W.synthetic_weights(0), "fp32", torch.float64, sites={s: 11 for s in oecapa.ROUNDING_SITES}).embed(feats)
    a, b = emb.double(), want.double()
    cos = (a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1))
    assert (cos > 1 - 2e-5 / 8).all(), 1 - cos
    assert torch.allclose(emb, want, rtol=0, atol=2e-3 * 2.0 ** -1.5 * float(want.abs().max())), float((emb - want).abs().max())
