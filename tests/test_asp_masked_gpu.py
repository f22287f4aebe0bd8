"""GPU checks of the masked attentive statistics pooling (csrc/asp_masked.hip) and of sdk_ecapa_forward_masked, in both 2-byte formats
(fmt 0 = bf16, 2 = fp16), against the float64 restatements of tests/asp_masked_ref.py on the same stored inputs.  Kernel level: every
element inside (want, bound), outputs in sentinel-filled wide buffers.  Whole forward: 1 - cos against MaskedEcapaOracle in float64 within
FACTOR x the reference's own fp32-vs-float64 spread.  Every case prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import asp_masked_ref as MR
import sweeps_ref as R
from conftest import sub

pytestmark = pytest.mark.gpu

L = sub("_lib")
W = sub("weights")
OPS = sub("ops")
DZ = sub("diarize")
SdkError = L.SdkError
FMTS = [0, 2]
SENT = -7.75
FACTOR = 3.0             # as tests/test_diarize_gpu.py
F_SEG = 589
SMALL = W.EcapaConfig(channels=256, mfa_channels=768, res2net_scale=2, se_channels=64, attn_channels=128)   # the smallest check_desc admits with 3 blocks


def _s():
    return torch.cuda.current_stream().cuda_stream


def _dev(x, fmt):
    return x.to(R.FMTS[fmt]).cuda()


def judge(got, want, bound, what):
    got = got.double().cpu()
    err = (got - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    bad = ~(err <= bound)
    print(f"{what}: worst err / bound {ratio:.3f}")
    assert not bad.any(), f"{what}: {int(bad.sum())} / {bad.numel()} outside the bound, worst err / bound {ratio:.3g}"


def stats_call(eng, h, B, T, w, valid, fmt, wide=True):
    Cm, S = h.shape[1], w.shape[1]
    if wide:
        buf = torch.full((B * S * 2 * Cm + 64,), SENT, dtype=torch.float32, device="cuda")
    else:
        buf = torch.empty((B * S * 2 * Cm,), dtype=torch.float32, device="cuda")
    L.check(eng.lib.sdk_asp_stats_masked_fmt(eng.ctx, h.data_ptr(), h.stride(0), B, T, Cm, S, w.data_ptr(), valid.data_ptr(), buf.data_ptr(), fmt, _s()),
            "sdk_asp_stats_masked_fmt")
    torch.cuda.synchronize()
    if wide:
        assert (buf[B * S * 2 * Cm:] == SENT).all(), "store outside the output"
    return buf[:B * S * 2 * Cm].reshape(B * S, 2 * Cm)


def pool_call(eng, lg, h, B, T, S, s, w, valid, fmt, out=None):
    Cm = h.shape[1]
    if out is None:
        out = torch.full((B * S, 2 * Cm), SENT, dtype=torch.float32, device="cuda")
    L.check(eng.lib.sdk_asp_pool_masked_fmt(eng.ctx, lg.data_ptr(), lg.stride(0), h.data_ptr(), h.stride(0), B, T, Cm, S, s, w.data_ptr(), valid.data_ptr(),
                                            out.data_ptr(), fmt, _s()), "sdk_asp_pool_masked_fmt")
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------- masked statistics
def _stat_weights(B, T, g):
    """two weight sets [B, 3, T] + valid: {ones, rand, one frame} and {last frame, all zero with valid = 0, rand}"""
    w1 = torch.stack([torch.ones(B, T), torch.rand(B, T, generator=g), torch.zeros(B, T)], 1)
    w1[:, 2, T // 2] = 1.0                                               # exactly one frame: std is the floor's 1e-6
    w2 = torch.stack([torch.zeros(B, T), torch.zeros(B, T), torch.rand(B, T, generator=g)], 1)
    w2[:, 0, T - 1] = 1.0                                                # only the last frame
    v1 = torch.ones(B, 3, dtype=torch.int32)
    v2 = torch.tensor([[1, 0, 1]] * B, dtype=torch.int32)
    return (w1, v1), (w2, v2)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("C", [8, 1032, 3072])
def test_masked_stats_sweep(engine, fmt, C):
    """tails of the 512-channel grid, ldh = C + 8, T on both sides of the 16-frame unrolled stripe; channels 0..7 at 1000 + N(0, 1)"""
    B = 2
    for T in (1, 2, 3, 201, 1001):
        g = torch.Generator().manual_seed(C + T)
        h = torch.randn(B * T, C, generator=g) * 3 + 1
        h[:, :8] = 1000 + torch.randn(B * T, 8, generator=g)
        h = R.store(h, fmt)
        hw = _dev(torch.cat([h, torch.full((B * T, 8), 3.0, dtype=torch.float64)], 1), fmt)[:, :C]
        for k, (w, valid) in enumerate(_stat_weights(B, T, g)):
            got = stats_call(engine, hw, B, T, w.cuda(), valid.cuda(), fmt)
            wz = w.clone()
            wz[valid == 0] = 0
            want, bound = MR.asp_stats_masked_ref(h, wz, B, T)
            judge(got, want, bound, f"asp_stats_masked fmt {fmt} C {C} T {T} set {k}")
            if k == 0:
                sd = got.cpu().reshape(B, 3, 2 * C)[:, 2, C:]
                assert float((sd - 1e-6).abs().max()) <= 1e-9, "one frame: std is sqrt(1e-12)"
            else:
                assert not got.cpu().reshape(B, 3, 2 * C)[:, 1].any(), "valid = 0: a zero row"


# ---------------------------------------------------------------------------------------------------- masked pooling
def _pool_data(B, T, C, fmt, seed):
    g = torch.Generator().manual_seed(seed)
    lg = (torch.rand(B * T, C, generator=g) * 160 - 80).float()
    lg[:, :8] = 1.5                                                     # exact ties
    lg[:, 8:16] = torch.randn(B * T, 8, generator=g)                    # one dominant frame (added below, on an active frame)
    h = R.store(torch.randn(B * T, C, generator=g) * (1e-5 if T == 2 else 2) + (0 if T == 2 else 3), fmt)     # T = 2: fp16 subnormals
    w = torch.rand(B, T, generator=g)
    w[:, ::3] = 0
    w[:, T // 2] = 0.7
    lg.view(B, T, C)[:, T // 2, 8:16] += 30
    return lg, h, w


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("C", [64, 192, 3072])
def test_masked_pool_sweep(engine, fmt, C):
    B, S, s = 2, 3, 1
    valid = torch.ones(B, S, dtype=torch.int32).cuda()
    for T in (1, 2, 225, 1001):
        lg, h, w = _pool_data(B, T, C, fmt, 7 * C + T)
        wall = torch.zeros(B, S, T)
        wall[:, s] = w
        wall[:, 0] = 1.0
        out = pool_call(engine, lg.cuda(), _dev(h, fmt), B, T, S, s, wall.cuda(), valid, fmt)
        o = out.cpu().reshape(B, S, 2 * C)
        assert (o[:, 0] == SENT).all() and (o[:, 2] == SENT).all(), "only the slot's rows are written"
        want, bound = MR.asp_pool_masked_ref(lg.double(), h, w, B, T)
        judge(o[:, s], want, bound, f"asp_pool_masked fmt {fmt} C {C} T {T}")


@pytest.mark.parametrize("fmt", FMTS)
def test_masked_pool_maximum_is_over_the_active_frames(engine, fmt):
    """frames with w = 0 hold +80 while every active frame holds at most -80: a maximum over all frames underflows every term (0 / 0).  The
    same case with the masked-out logits NaN and +inf is bit-identical."""
    B, T, C = 2, 225, 192
    g = torch.Generator().manual_seed(3)
    h = R.store(torch.randn(B * T, C, generator=g) * 2 + 3, fmt)
    w = (torch.rand(B, T, generator=g) < 0.4).float()
    w[:, 0], w[:, 5] = 0.0, 1.0
    act = (w > 0).reshape(B * T)
    lg = torch.where(act[:, None], -80 - 20 * torch.rand(B * T, C, generator=g), torch.full((B * T, C), 80.0)).float()
    valid = torch.ones(B, 1, dtype=torch.int32).cuda()
    outs = []
    for fill in (80.0, float("nan"), float("inf")):
        l2 = lg.clone()
        l2[~act] = fill
        outs.append(pool_call(engine, l2.cuda(), _dev(h, fmt), B, T, 1, 0, w.reshape(B, 1, T).cuda(), valid, fmt).cpu())
    want, bound = MR.asp_pool_masked_ref(lg.double(), h, w, B, T)
    judge(outs[0], want, bound, f"asp_pool_masked fmt {fmt} masked-out +80")
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), "a masked-out logit changed the result"
    # no active frame at all, valid != 0: zeros; valid = 0: zeros, weights unread
    z = pool_call(engine, lg.cuda(), _dev(h, fmt), B, T, 1, 0, torch.zeros(B, 1, T).cuda(), valid, fmt).cpu()
    z2 = pool_call(engine, lg.cuda(), _dev(h, fmt), B, T, 1, 0, torch.full((B, 1, T), float("nan")).cuda(), torch.zeros(B, 1, dtype=torch.int32).cuda(), fmt).cpu()
    assert not z.any() and not z2.any()


@pytest.mark.parametrize("fmt", FMTS)
def test_all_ones_weights_against_the_unmasked_kernels(engine, fmt):
    B, T, C = 2, 501, 1024
    g = torch.Generator().manual_seed(11)
    h = R.store(torch.randn(B * T, C, generator=g) * 2 + 1, fmt)
    lg = (torch.rand(B * T, C, generator=g) * 40 - 20).float()
    hd, lgd = _dev(h, fmt), lg.cuda()
    ones, valid = torch.ones(B, 1, T).cuda(), torch.ones(B, 1, dtype=torch.int32).cuda()
    st = torch.empty((B, 2 * C), dtype=torch.float32, device="cuda")
    L.check(engine.lib.sdk_asp_stats_fmt(engine.ctx, hd.data_ptr(), hd.stride(0), B, T, C, st.data_ptr(), fmt, _s()), "sdk_asp_stats_fmt")
    pl = torch.empty((B, 2 * C), dtype=torch.float32, device="cuda")
    L.check(engine.lib.sdk_asp_pool_fmt(engine.ctx, lgd.data_ptr(), lgd.stride(0), hd.data_ptr(), hd.stride(0), B, T, C, pl.data_ptr(), fmt, _s()), "sdk_asp_pool_fmt")
    mst = stats_call(engine, hd, B, T, ones, valid, fmt)
    mpl = pool_call(engine, lgd, hd, B, T, 1, 0, ones, valid, fmt)
    want, bound = R.asp_stats_ref(h, B, T)
    judge(st, want, bound, f"sdk_asp_stats_fmt fmt {fmt}")
    mwant, mbound = MR.asp_stats_masked_ref(h, torch.ones(B, 1, T), B, T)
    assert float((want - mwant).abs().max()) <= 1e-12
    judge(mst, mwant, mbound, f"asp_stats_masked w = 1 fmt {fmt}")
    want, bound = R.asp_pool_ref(lg.double(), h, B, T)
    judge(pl, want, bound, f"sdk_asp_pool_fmt fmt {fmt}")
    mwant, mbound = MR.asp_pool_masked_ref(lg.double(), h, torch.ones(B, T), B, T)
    assert float((want - mwant).abs().max()) <= 1e-12
    judge(mpl, mwant, mbound, f"asp_pool_masked w = 1 fmt {fmt}")


@pytest.mark.parametrize("fmt", FMTS)
def test_kernel_rows_depend_on_their_own_weights_only(engine, fmt):
    B, T, C, S = 2, 201, 192, 3
    g = torch.Generator().manual_seed(13)
    h = _dev(R.store(torch.randn(B * T, C, generator=g) * 2 + 1, fmt), fmt)
    lg = (torch.rand(B * T, C, generator=g) * 20 - 10).float().cuda()
    w = torch.rand(B, S, T, generator=g)
    w2 = w.clone()
    w2[:, 0] = torch.rand(B, T, generator=g)
    w2[:, 2] = 1.0
    valid = torch.ones(B, S, dtype=torch.int32).cuda()
    a, a2, b = (stats_call(engine, h, B, T, x.cuda(), valid, fmt).cpu().reshape(B, S, -1) for x in (w, w, w2))
    assert torch.equal(a, a2), "two runs differ"
    assert torch.equal(a[:, 1], b[:, 1]) and not torch.equal(a[:, 0], b[:, 0])
    p, p2, q = (pool_call(engine, lg, h, B, T, S, 1, x.cuda(), valid, fmt).cpu().reshape(B, S, -1) for x in (w, w, w2))
    assert torch.equal(p, p2), "two runs differ"
    assert torch.equal(p[:, 1], q[:, 1])


# ---------------------------------------------------------------------------------------------------- the whole forward
def random_cls(rng, Cn, p_sil=0.2):
    cls = np.zeros((Cn, F_SEG), np.uint8)
    for c in range(Cn):
        i = 0
        while i < F_SEG:
            n = int(rng.integers(1, 90))
            cls[c, i:i + n] = 0 if rng.random() < p_sil else rng.integers(1, 7)
            i += n
    return cls


def one_cos(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 1.0 - (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


_ENGINES = {}


def _engine(cfg_name, fmt):
    """engines of the two configurations (no bias correction: the plain layer-boundary model), per format"""
    key = (cfg_name, fmt)
    if key not in _ENGINES:
        cfg = W.DEFAULT_CONFIG if cfg_name == "default" else SMALL
        seed = 0 if cfg_name == "default" else 3
        e = OPS.Engine(0, W.synthetic_weights(seed, cfg), cfg, bias_correction=False)
        e.set_precision(fmt)
        _ENGINES[key] = (e, W.synthetic_weights(seed, cfg), cfg)
    return _ENGINES[key]


def _feats(B, T, fmt, seed):
    g = torch.Generator().manual_seed(seed)
    f = R.store(torch.randn(B, T, 80, generator=g), fmt)
    dev = torch.zeros(B * T, 128, dtype=R.FMTS[fmt])
    dev[:, :80] = f.reshape(B * T, 80).to(R.FMTS[fmt])
    return f.float(), dev.cuda()


_FWD = {}


def _forward_case(cfg_name, fmt, B, T):
    """(device embeddings [B, 3, d], a second run, oracle float64, oracle fp32 accumulation, valid) - computed once, shared"""
    key = (cfg_name, fmt, B, T)
    if key not in _FWD:
        eng, wts, cfg = _engine(cfg_name, fmt)
        fh, fd = _feats(B, T, fmt, 17 + T)
        cls = random_cls(np.random.default_rng(3), B)
        w, info = DZ.diarize_masks(eng, torch.from_numpy(cls).cuda(), T)
        valid = info[:, :, 3].contiguous()
        got = eng.ecapa_forward_masked(fd, B, T, w, valid)
        got2 = eng.ecapa_forward_masked(fd, B, T, w, valid)
        torch.cuda.synchronize()
        sites = {s: R.BITS[fmt] for s in MR.oecapa.ROUNDING_SITES}
        kw = dict(n_dilations=cfg.dilations, scale=cfg.res2net_scale, sites=sites)
        e64 = MR.MaskedEcapaOracle(wts, "fp32", torch.float64, **kw).embed_masked(fh, w.cpu())
        e32 = MR.MaskedEcapaOracle(wts, "fp32", torch.float32, **kw).embed_masked(fh, w.cpu())
        _FWD[key] = (got.cpu(), got2.cpu(), e64.numpy(), e32.numpy(), valid.cpu().numpy().astype(bool), (eng, fd, w, valid))
    return _FWD[key]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("cfg_name,B,T", [("default", 2, 1001), ("small", 1, 225)])
def test_masked_forward_against_the_masked_oracle(cfg_name, B, T, fmt):
    got, got2, e64, e32, ok, _ = _forward_case(cfg_name, fmt, B, T)
    assert torch.equal(got, got2), "two runs differ"
    assert int(ok.sum()) >= (4 if B > 1 else 1)
    g = got.numpy().reshape(B, 3, -1)
    spread = float(one_cos(e32, e64)[ok].max())
    err = float(one_cos(g, e64)[ok].max())
    print(f"masked ECAPA forward {cfg_name} fmt {fmt} B {B} T {T}: oracle fp32-vs-float64 spread (1 - cos) {spread:.3e} bound {FACTOR * spread:.3e} gpu {err:.3e}")
    assert np.isfinite(err) and err <= FACTOR * spread
    assert not g[~ok].any(), "valid = 0 rows must be zeros"


@pytest.mark.parametrize("fmt", FMTS)
def test_forward_rows_depend_on_their_own_weights_only(fmt):
    B, T = 2, 1001
    got, _, _, _, ok, (eng, fd, w, valid) = _forward_case("default", fmt, B, T)
    w2 = w.clone()
    w2[:, 0] = torch.rand(B, T, device="cuda")
    w2[:, 2] = 1.0
    e2 = eng.ecapa_forward_masked(fd, B, T, w2, valid).cpu().reshape(B, 3, -1)
    e1 = got.reshape(B, 3, -1)
    assert torch.equal(e1[:, 1], e2[:, 1]), "slot 1's rows changed with the other slots' weights"
    assert ok[:, 0].any() and not torch.equal(e1[:, 0], e2[:, 0])


@pytest.mark.parametrize("fmt", FMTS)
def test_all_ones_forward_against_sdk_ecapa_forward(fmt):
    """S = 1, w = 1 against sdk_ecapa_forward on the same features: the same trunk bit for bit; the context statistics come from another
    fp32 reduction (the MFA epilogue's column sums against the masked sweep) and the pooling from asp_pool_kernel against its masked twin.
    Kernel-level bounds (test_all_ones_weights_against_the_unmasked_kernels): both statistics lie within n 2^-24 sum|terms| / v1 of
    float64, n ~ 1e3 -> <= 1.2e-4 relative to the mean magnitude, for two kernels 2.4e-4 apart at the very worst.  That moves ubias, hence a
    hidden value by at most that (BN gain ~ 1, tanh' <= 1) plus one flip of its 2-byte rounding, 2^-8 (bf16) / 2^-11 (fp16) relative, on a
    small fraction of elements; a pooled row moves by no more than the larger of the two, r <= 2^-8 + 2.4e-4 = 4.2e-3 (bf16), 7.3e-4
    (fp16), relative - taking EVERY element at its worst.  1 - cos is quadratic in a row's relative displacement; with the factor 3 for the
    final FC's conditioning that test_masked_forward_consistency uses: (3 r)^2 / 2 = 8e-5 (bf16), 2.4e-6 (fp16)."""
    B, T = 2, 1001
    eng, _, _ = _engine("default", fmt)
    _, fd = _feats(B, T, fmt, 17 + T)
    a = eng.ecapa_forward_masked(fd, B, T, torch.ones(B, 1, T, device="cuda"), torch.ones(B, 1, dtype=torch.int32, device="cuda")).cpu().numpy()
    b = eng.ecapa_forward(fd, B, T).cpu().numpy()
    d = float(one_cos(a, b).max())
    bound = {0: 8e-5, 2: 2.4e-6}[fmt]
    print(f"all-ones masked forward vs sdk_ecapa_forward fmt {fmt}: 1 - cos {d:.3e} (bound {bound:.1e})")
    assert d <= bound


def test_refusals(engine):
    eng, _, _ = _engine("default", 0)
    B, T, S = 1, 225, 3
    _, fd = _feats(B, T, 0, 1)
    d = eng.desc
    w = torch.ones(B, S, T, device="cuda")
    valid = torch.ones(B, S, dtype=torch.int32, device="cuda")
    need = eng.lib.sdk_ecapa_masked_workspace_bytes(C.byref(d), B, T, S)
    assert need > eng.lib.sdk_ecapa_workspace_bytes(C.byref(d), B, T)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    emb = torch.empty((B * S, 192), dtype=torch.float32, device="cuda")

    def call(desc=d, S_=S, wp=w.data_ptr(), nbytes=need, T_=T):
        L.check(eng.lib.sdk_ecapa_forward_masked(eng.ctx, eng._wblob.data_ptr(), C.byref(desc), fd.data_ptr(), fd.stride(0), B, T_, S_, wp, valid.data_ptr(),
                                                 ws.data_ptr(), nbytes, emb.data_ptr(), _s()), "sdk_ecapa_forward_masked")
    d1 = L.EcapaDesc.from_buffer_copy(d)
    d1.precision = 1
    d1.n_mels_padded = 96
    with pytest.raises(SdkError, match="precision 1 .* not built for the masked pooling"):
        call(desc=d1)
    with pytest.raises(SdkError, match=r"S=0 weight rows per chunk \(served: 1 .. 8\)"):
        call(S_=0)
    with pytest.raises(SdkError, match=r"S=9 weight rows per chunk \(served: 1 .. 8\)"):
        call(S_=9)
    with pytest.raises(SdkError, match=rf"workspace of {need - 256} bytes, {need} needed \(sdk_ecapa_masked_workspace_bytes\)"):
        call(nbytes=need - 256)
    with pytest.raises(SdkError, match=r"null pointer \(w=\(nil\)"):
        call(wp=None)
    with pytest.raises(SdkError, match="shorter than the receptive halo 4"):
        call(T_=4)
    h = torch.zeros(8, 64, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(2, 128, device="cuda")
    with pytest.raises(SdkError, match="sdk_asp_stats_masked_fmt: precision=1"):
        L.check(eng.lib.sdk_asp_stats_masked_fmt(eng.ctx, h.data_ptr(), 64, 1, 8, 64, 1, w.data_ptr(), valid.data_ptr(), out.data_ptr(), 1, _s()), "stats")
    with pytest.raises(SdkError, match="sdk_asp_pool_masked_fmt: precision=1"):
        L.check(eng.lib.sdk_asp_pool_masked_fmt(eng.ctx, out.data_ptr(), 64, h.data_ptr(), 64, 1, 8, 64, 1, 0, w.data_ptr(), valid.data_ptr(), out.data_ptr(), 1, _s()), "pool")
    with pytest.raises(SdkError, match=r"sdk_asp_stats_masked: S=9"):
        L.check(eng.lib.sdk_asp_stats_masked_fmt(eng.ctx, h.data_ptr(), 64, 1, 8, 64, 9, w.data_ptr(), valid.data_ptr(), out.data_ptr(), 0, _s()), "stats")
    with pytest.raises(ValueError, match="w must be a contiguous fp32 device tensor"):
        eng.ecapa_forward_masked(fd, B, T, w.double(), valid)
    with pytest.raises(ValueError, match="valid must be a contiguous int32 device tensor"):
        eng.ecapa_forward_masked(fd, B, T, w, valid.long())
    call()                                                              # the device is fine after the refusals
    torch.cuda.synchronize()
    assert torch.isfinite(emb).all()
