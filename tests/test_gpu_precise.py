"""The PRECISE mode (sdk_set_option "precision" 1, csrc/hp.hip): fp16 hi+lo planes, three MFMAs per product.  VERDICT r2 next #1c:
north_star asks for cosine scores within 1e-5 of the fp32 model and identical IDs; the default bf16 mode is 4e-3 away and the error
budget (profiles/r03_error_budget.md) says every rounding site needs ~18+ significand bits.  Here: the split GEMM against float64 on
the values it actually multiplies, the split fbank, the whole C = 1024 forward against the UN-ROUNDED oracle, and PCM -> score on
config #2's first 64 segments x 100 profiles with the bound asserted at 1e-5."""
import json

import numpy as np
import pytest
import torch

from conftest import ROOT, sub
from oracle import ecapa as oecapa
from oracle import fbank as ofbank

pytestmark = pytest.mark.gpu

W = sub("weights")
WP = sub("weights_pack")
OPS = sub("ops")


@pytest.fixture()
def precise(engine):
    engine.set_precision(1)
    yield engine
    engine.set_precision(0)


def _conv_ref64(A, Wt, Cin, taps, dil, T):
    A = A.double()
    M = A.shape[0]
    B = M // T
    t = torch.arange(T)
    out = torch.zeros(M, Wt.shape[0], dtype=torch.float64)
    mag = torch.zeros_like(out)
    Ab = A.reshape(B, T, -1)[:, :, :Cin]
    for j in range(taps):
        src = oecapa.reflect_index(t + (j - taps // 2) * dil, T)
        a = Ab[:, src, :].reshape(M, Cin)
        w = Wt.double()[:, j * Cin:(j + 1) * Cin]
        out += a @ w.T
        mag += a.abs() @ w.abs().T
    return out, mag


@pytest.mark.parametrize("M,T,N,Cin,taps,dil,scale_a,scale_w", [
    (512, 512, 128, 64, 1, 1, 1.0, 0.05),
    (603, 201, 256, 128, 3, 2, 1.0, 0.03),
    (1005, 201, 1024, 96, 5, 1, 8.0, 0.1),         # blk0's shape: mel planes padded to 96
    (402, 201, 128, 1024, 1, 1, 0.01, 0.03),       # small activations: the scaled lo plane keeps its precision (unscaled: 2e-6)
    (256, 256, 384, 3072, 1, 1, 3.0, 1e-4),        # tiny weights: the per-layer power-of-two scale
])
def test_conv_gemm_hp_matches_float64(precise, M, T, N, Cin, taps, dil, scale_a, scale_w):
    eng = precise
    g = torch.Generator().manual_seed(M + N + Cin)
    a = torch.randn(M, Cin, generator=g) * scale_a
    w = torch.randn(N, taps * Cin, generator=g) * scale_w
    Ap = OPS.Engine.to_planes(a)
    slot = WP.hp_weight_planes(w.numpy())
    a_eff = OPS.Engine.from_planes(Ap)                                # what the planes hold (22+ bits of a)
    w_eff = torch.from_numpy(WP.hp_planes_to_f64(slot, N, taps * Cin))
    assert float((a_eff - a).abs().max()) <= 2.0 ** -21 * float(a.abs().max())
    assert float((w_eff - w.double()).abs().max()) <= 2.0 ** -21 * float(w.abs().max())
    Cp, C32, _ = eng.conv_gemm_hp(Ap.cuda(), torch.from_numpy(slot.view(np.int16)).cuda(), N, Cin, taps=taps, dil=dil, T=T, out_f32=True)
    torch.cuda.synchronize()
    ref, mag = _conv_ref64(a_eff, w_eff, Cin, taps, dil, T)
    err = (C32.cpu().double() - ref).abs()
    # dropped lo.lo term: 2^-22 per product; fp32 accumulation over K: ~sqrt(K) 2^-24 of the running sum
    assert float((err / mag).max()) < 1.5e-6, float((err / mag).max())
    assert float(err.max()) < 3e-6 * float(ref.abs().max()) + 1e-30
    # the planes output decodes to the fp32 output within the pair's 22 bits
    back = OPS.Engine.from_planes(Cp.cpu())
    assert float((back - C32.cpu()).abs().max()) <= 2.0 ** -21 * float(C32.abs().max())


@pytest.mark.parametrize("M,T,N,Cin,taps,dil", [
    (1005, 201, 1024, 96, 5, 1),          # blk0: taps, 15 K-steps of 32, partial last m-tile (the per-row clamp path)
    (2010, 201, 1024, 1024, 1, 1),        # a TDNN layer: 8 m-tiles x 4 n-tiles
    (515, 515, 256, 3072, 1, 1),          # long K, M = 2 tiles + 3 rows
    (256, 256, 512, 64, 1, 1),            # two K-steps: prologue / last-step paths only
    (768, 256, 256, 32, 1, 1),            # a single K-step
    (603, 201, 256, 128, 3, 2),           # dilated taps across segment boundaries inside a tile
])
def test_conv_gemm_hp_256_tile_kernel(precise, M, T, N, Cin, taps, dil):
    """The precise mode's big layers run on a 256 x 256 LDS-DMA tile (conv_gemm_hp256_kernel: hi | lo halves of a 128-byte LDS row, six MFMA
    sub-phases per 32-wide K-step, hi then lo plane through the tile image).  Planes out vs float64 on the values the planes hold, and
    against the 128^2 register-staged kernel (knob hp_gemm_variant 1) on the same operands."""
    eng = precise
    g = torch.Generator().manual_seed(M + N + Cin + taps)
    a = torch.randn(M, Cin, generator=g) * 2.0
    w = torch.randn(N, taps * Cin, generator=g) * 0.04
    bias, sc, sh = torch.randn(N, generator=g), torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
    Ap = OPS.Engine.to_planes(a)
    slot = WP.hp_weight_planes(w.numpy())
    Wd = torch.from_numpy(slot.view(np.int16)).cuda()
    dv = lambda t: t.cuda()
    out = {}
    for variant in (0, 1):
        eng.set_option("hp_gemm_variant", variant)
        try:
            Cp, _, _ = eng.conv_gemm_hp(dv(Ap), Wd, N, Cin, taps=taps, dil=dil, T=T, bias=dv(bias), scale=dv(sc), shift=dv(sh), relu=True)
            torch.cuda.synchronize()
        finally:
            eng.set_option("hp_gemm_variant", 0)
        out[variant] = OPS.Engine.from_planes(Cp.cpu()).double()
    pre, mag = _conv_ref64(OPS.Engine.from_planes(Ap), torch.from_numpy(WP.hp_planes_to_f64(slot, N, taps * Cin)), Cin, taps, dil, T)
    want = torch.relu(pre + bias.double()) * sc.double() + sh.double()
    tol = 1.5e-6 * mag * sc.double() + 2.0 ** -21 * want.abs() + 1e-7
    for variant in (0, 1):
        err = (out[variant] - want).abs()
        assert (err <= tol).all(), (variant, float((err / tol).max()), float(err.max()))
    assert float((out[0] - out[1]).abs().max()) <= 3e-6 * float(want.abs().max())


# (M, T, N, Cin, taps, dil): segments shorter than a tile and the dispatch rule's edges (taps > 1 && T < 64, or M < 256 -> the 128^2 kernel)
SHORT_SEGMENT_SHAPES = [
    (1, 1, 128, 32, 1, 1),              # the smallest call
    (9, 9, 128, 64, 3, 4),              # a short segment with a dilated halo
    (18, 9, 128, 128, 3, 4),            # two short segments in one tile
    (3, 3, 128, 32, 3, 2),              # halo = T - 1
    (150, 50, 256, 96, 5, 1),           # five taps, a partial m-tile
    (640, 40, 256, 128, 3, 3),          # M >= 256 but T < 64: the 128^2 kernel
    (256, 64, 256, 64, 3, 4),           # the dispatch edge T = 64: four segments inside one 256-row tile
    (260, 65, 256, 64, 3, 3),           # one full 256-row tile plus a partial tile of 4 live rows
]


@pytest.mark.parametrize("M,T,N,Cin,taps,dil", SHORT_SEGMENT_SHAPES)
def test_conv_gemm_hp_short_segments(precise, M, T, N, Cin, taps, dil):
    """sdk_conv_gemm_hp where the forward's shortest windows put it: segment-local reflection with several segment boundaries inside one
    tile, tiles of mostly clamped rows, both sides of the 256^2 kernel's dispatch rule.  The fp32 output by the method and tolerances of
    test_conv_gemm_hp_matches_float64, the planes with the full epilogue by those of test_conv_gemm_hp_256_tile_kernel in both
    hp_gemm_variant 0 and 1; where the rule keeps the 256^2 kernel out, variant 0 must BE the 128^2 kernel: the same bits."""
    eng = precise
    g = torch.Generator().manual_seed(M + N + Cin + taps)
    a = torch.randn(M, Cin, generator=g) * 2.0
    w = torch.randn(N, taps * Cin, generator=g) * 0.04
    bias, sc, sh = torch.randn(N, generator=g), torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
    Ap = OPS.Engine.to_planes(a)
    slot = WP.hp_weight_planes(w.numpy())
    Wd = torch.from_numpy(slot.view(np.int16)).cuda()
    pre, mag = _conv_ref64(OPS.Engine.from_planes(Ap), torch.from_numpy(WP.hp_planes_to_f64(slot, N, taps * Cin)), Cin, taps, dil, T)
    shape = f"conv_gemm_hp M {M} T {T} N {N} Cin {Cin} taps {taps} dil {dil}"
    # the bare product, fp32 out
    Cp, C32, _ = eng.conv_gemm_hp(Ap.cuda(), Wd, N, Cin, taps=taps, dil=dil, T=T, out_f32=True)
    torch.cuda.synchronize()
    err = (C32.cpu().double() - pre).abs()
    print(f"{shape} fp32 out: worst err / tol {float((err / mag).max()) / 1.5e-6:.3f}")
    assert float((err / mag).max()) < 1.5e-6, float((err / mag).max())
    assert float(err.max()) < 3e-6 * float(pre.abs().max()) + 1e-30
    assert float((OPS.Engine.from_planes(Cp.cpu()) - C32.cpu()).abs().max()) <= 2.0 ** -21 * float(C32.abs().max())
    # planes out with bias / ReLU / BN affine, both kernels where both are eligible
    out, bits = {}, {}
    for variant in (0, 1):
        eng.set_option("hp_gemm_variant", variant)
        try:
            Cp, _, _ = eng.conv_gemm_hp(Ap.cuda(), Wd, N, Cin, taps=taps, dil=dil, T=T, bias=bias.cuda(), scale=sc.cuda(), shift=sh.cuda(), relu=True)
            torch.cuda.synchronize()
        finally:
            eng.set_option("hp_gemm_variant", 0)
        bits[variant] = Cp.cpu()
        out[variant] = OPS.Engine.from_planes(bits[variant]).double()
    want = torch.relu(pre + bias.double()) * sc.double() + sh.double()
    tol = 1.5e-6 * mag * sc.double() + 2.0 ** -21 * want.abs() + 1e-7
    for variant in (0, 1):
        err = (out[variant] - want).abs()
        print(f"{shape} planes out variant {variant}: worst err / tol {float((err / tol).max()):.3f}")
        assert (err <= tol).all(), (variant, float((err / tol).max()), float(err.max()))
    assert float((out[0] - out[1]).abs().max()) <= 3e-6 * float(want.abs().max())
    if not (M >= 256 and N % 256 == 0 and (taps == 1 or T >= 64)):
        assert torch.equal(bits[0].view(torch.int16), bits[1].view(torch.int16)), "the 256^2 kernel ran outside its dispatch rule"


@pytest.mark.parametrize("M,T,N,Cin,taps,dil", [(40200, 201, 1024, 64, 1, 1), (20100, 201, 1024, 96, 3, 2), (66000, 200, 1024, 32, 1, 1), (40200, 201, 2048, 32, 1, 1)])
def test_conv_gemm_hp_half_tile_tail_is_bit_identical(precise, M, T, N, Cin, taps, dil):
    """Round 5: the precise GEMM's 256^2 kernel computes a mostly idle last tile round as 128 x 256 half tiles (as conv_gemm256_kernel does): the
    same three product terms in the same K order per element, so both planes must equal the whole-tile schedule's (hp_gemm_variant 2 = half
    tiles off) bit for bit - taps across segment boundaries, an edge half tile, and a shape the rule leaves alone (N = 2048)."""
    eng = precise
    g = torch.Generator().manual_seed(M + N + Cin + taps)
    a = torch.randn(M, Cin, generator=g) * 2.0
    w = torch.randn(N, taps * Cin, generator=g) * 0.04
    bias, sc, sh = torch.randn(N, generator=g), torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
    Ap = OPS.Engine.to_planes(a).cuda()
    Wd = torch.from_numpy(WP.hp_weight_planes(w.numpy()).view(np.int16)).cuda()
    out = {}
    for variant in (0, 2):
        eng.set_option("hp_gemm_variant", variant)
        try:
            out[variant] = eng.conv_gemm_hp(Ap, Wd, N, Cin, taps=taps, dil=dil, T=T, bias=bias.cuda(), scale=sc.cuda(), shift=sh.cuda(), relu=True)[0]
            torch.cuda.synchronize()
        finally:
            eng.set_option("hp_gemm_variant", 0)
    assert torch.equal(out[0].view(torch.int16), out[2].view(torch.int16))
    if taps == 1:      # and against float64 on a sample of rows from the tail region
        rows = torch.arange(M - 300, M)
        want = torch.relu(OPS.Engine.from_planes(Ap[rows].cpu()).double() @ torch.from_numpy(WP.hp_planes_to_f64(WP.hp_weight_planes(w.numpy()), N, Cin)).T + bias.double()) * sc.double() + sh.double()
        got = OPS.Engine.from_planes(out[0][rows].cpu()).double()
        assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_conv_gemm_hp_epilogue_and_residual_sum(precise):
    eng = precise
    M, T, N, Cin = 402, 201, 128, 128
    g = torch.Generator().manual_seed(5)
    a = torch.randn(M, Cin, generator=g)
    w = torch.randn(N, 3 * Cin, generator=g) * 0.05
    bias, sc, sh = torch.randn(N, generator=g), torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
    ub = torch.randn(M // T, N, generator=g)
    x2 = torch.randn(M, N, generator=g)
    Ap, X2p = OPS.Engine.to_planes(a), OPS.Engine.to_planes(x2)
    slot = WP.hp_weight_planes(w.numpy())
    dv = lambda t: t.cuda()
    Cp, C32, Sp = eng.conv_gemm_hp(dv(Ap), torch.from_numpy(slot.view(np.int16)).cuda(), N, Cin, taps=3, dil=3, T=T, bias=dv(bias), scale=dv(sc),
                                   shift=dv(sh), ubias=dv(ub), relu=True, tanh=True, out_f32=True, X2=dv(X2p))
    torch.cuda.synchronize()
    pre, _ = _conv_ref64(OPS.Engine.from_planes(Ap), torch.from_numpy(WP.hp_planes_to_f64(slot, N, 3 * Cin)), Cin, 3, 3, T)
    want = torch.tanh(torch.relu(pre + bias.double() + ub.double().repeat_interleave(T, 0)) * sc.double() + sh.double())
    assert float((C32.cpu().double() - want).abs().max()) < 2e-6
    s_want = want + OPS.Engine.from_planes(X2p).double()
    assert float((OPS.Engine.from_planes(Sp.cpu()).double() - s_want).abs().max()) < 4e-6


def test_fbank_precise_mode(precise):
    eng = precise
    import importlib, sys
    sys.path.insert(0, str(ROOT))
    bench = importlib.import_module("bench")
    pcm = bench.synth_pcm(6, seed=3)
    feats = eng.fbank(torch.from_numpy(pcm).cuda())
    torch.cuda.synchronize()
    T = 201
    assert feats.dtype == torch.float16 and feats.shape == (6 * T, 192)
    got = OPS.Engine.from_planes(feats.cpu()).double().reshape(6, T, 96)
    assert not got[:, :, 80:].any()
    want = torch.from_numpy(ofbank.fbank(pcm)).double()
    # What fp32 accumulation can promise: a DFT bin is a sum of ~200 terms of the size of the LOUDEST component of the frame, so a quiet
    # bin next to a loud one (mel 0 at -41 dB beside a 0.2-amplitude sinusoid) carries an absolute error of ~2^-24 of that size:
    # |d dB| ~ 4.35 * 2 * 2^-24 * sqrt(loudest mel power of the frame / this mel power)  (measured: tools/fbank_hp_debug.py - max 6.6e-4 dB
    # at exactly such a bin, median 6e-7 dB; the default mode's bf16 x 3 table: 3.7e-3 / 1.3e-5).  Tolerance = twice the measured worst ratio.
    Mp = torch.from_numpy(ofbank.power_spectrum(pcm) @ ofbank.mel_matrix())
    tol = 4e-6 + 3.4e-6 * torch.sqrt(Mp.max(dim=2, keepdim=True).values / Mp.clamp_min(1e-10))      # (measured worst: 0.5 of this)
    err = (got[:, :, :80] - want).abs()
    # (the per-bin mean over frames is subtracted on both sides: its own error is an average of the above, far inside the tolerance)
    assert (err <= tol + 2e-6).all(), (float(err.max()), float((err / tol).max()))
    assert float(err.median()) < 3e-6 and float(err.flatten().kthvalue(int(0.999 * err.numel())).values) < 1e-4


def test_ecapa_forward_precise_vs_unrounded_oracle(precise):
    """C = 1024, 4 two-second segments: embeddings against the fp32 model with float64 accumulation (no rounding anywhere)."""
    eng = precise
    weights = W.synthetic_weights(0)
    g = torch.Generator().manual_seed(22)
    feats = torch.randn(4, 201, 80, generator=g) * 4.0
    f96 = torch.zeros(4 * 201, 96)
    f96[:, :80] = feats.reshape(-1, 80)
    emb = eng.ecapa_forward(OPS.Engine.to_planes(f96).cuda(), 4, 201).cpu()
    want = oecapa.EcapaOracle(weights, "fp32", torch.float64).embed(feats)
    a, b = emb.double(), want.double()
    cos = (a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1))
    assert (1 - cos).max() < 1e-11, (1 - cos).max()
    assert float((emb - want).abs().max()) < 3e-6 * float(want.abs().max())


PRECISE_SCORE_BOUND = 1e-5          # north_star: "cosine scores within 1e-5 fp32"


def _unit_profiles():
    import importlib, sys
    sys.path.insert(0, str(ROOT))
    return torch.from_numpy(importlib.import_module("bench").unit_rows(100, 192, seed=1)).double()


def _judge_embeddings(emb, want, what):
    """the forward test's element-wise criterion and the product's own: every cosine score against 100 seeded unit profiles within 1e-5"""
    a, b = emb.double(), want.double()
    assert not torch.isnan(a).any()
    d_el = float((a - b).abs().max()) / float(b.abs().max())
    P = _unit_profiles()
    d_score = float(((a / a.norm(dim=1, keepdim=True)) @ P.T - (b / b.norm(dim=1, keepdim=True)) @ P.T).abs().max())
    print(f"{what}: max |d emb| / max |emb| {d_el:.3g} (bound 3e-6), max |d score| {d_score:.3g} (bound {PRECISE_SCORE_BOUND:g}): "
          f"worst err / bound {max(d_el / 3e-6, d_score / PRECISE_SCORE_BOUND):.3f}")
    return d_el, d_score


@pytest.mark.parametrize("B,T", [(3, 50), (2, 9), (1, 201), (2, 301)])
@pytest.mark.parametrize("cfg_name", ["full", "small"])
def test_ecapa_forward_precise_off_its_one_shape(precise, cfg_name, B, T):
    """the whole precise forward at the window lengths the default mode's forward is tested at (short segments: the 128^2 GEMM and the
    sweeps' T < 8 paths; 301: past one ASP block), C = 1024 and test_gpu_kernels' small configuration, against the un-rounded oracle"""
    from test_gpu_kernels import SMALL
    g = torch.Generator().manual_seed(40 + T)
    feats = torch.randn(B, T, 80, generator=g) * 4.0
    f96 = torch.zeros(B * T, 96)
    f96[:, :80] = feats.reshape(-1, 80)
    if cfg_name == "full":
        eng, weights = precise, W.synthetic_weights(0)
        orc = oecapa.EcapaOracle(weights, "fp32", torch.float64)
    else:
        weights = W.synthetic_weights(3, SMALL)
        eng = OPS.Engine(0, weights=weights, cfg=SMALL, bias_correction=False)
        eng.set_precision(1)
        orc = oecapa.EcapaOracle(weights, "fp32", torch.float64, n_dilations=SMALL.dilations, scale=SMALL.res2net_scale)
    emb = eng.ecapa_forward(OPS.Engine.to_planes(f96).cuda(), B, T).cpu()
    want = orc.embed(feats)
    d_el, d_score = _judge_embeddings(emb, want, f"precise ecapa forward {cfg_name} B {B} T {T}")
    assert float((emb - want).abs().max()) < 3e-6 * float(want.abs().max())
    assert d_score <= PRECISE_SCORE_BOUND


@pytest.mark.parametrize("B,T", [(3, 50), (1, 20), (2, 301)])
def test_xvector_forward_precise_off_its_one_shape(engine, B, T):
    """the x-vector family's precise forward at feature level (planes in, sdk_conv_gemm_hp per frame layer, asp_stats_hp pooling)
    against the fp32 model with float64 accumulation: the 1e-5 score criterion of test_xvector_precise_mode_meets_1e5"""
    from oracle import xvector as oxv
    XV = sub("xvector")
    w = XV.synthetic_weights(0)
    xv = XV.XVector(engine, w, precision=1)
    g = torch.Generator().manual_seed(60 + T)
    feats = torch.randn(B, T, 80, generator=g) * 3.0
    f96 = torch.zeros(B * T, 96)
    f96[:, :80] = feats.reshape(-1, 80)
    emb = xv.forward(OPS.Engine.to_planes(f96).cuda(), B, T).cpu()
    want = oxv.xvector_embed(w, feats, mode="fp32", acc=torch.float64)
    _, d_score = _judge_embeddings(emb, want, f"precise x-vector forward B {B} T {T}")
    assert d_score <= PRECISE_SCORE_BOUND


def test_pcm_to_score_within_1e5_in_precise_mode(precise):
    """The criterion itself: PCM -> fbank -> ECAPA -> L2 -> cosine vs 100 profiles on config #2's first 64 segments, against the
    un-rounded oracle: every one of the 6400 scores within 1e-5, every argmax ID identical."""
    eng = precise
    import importlib, sys
    sys.path.insert(0, str(ROOT))
    bench = importlib.import_module("bench")
    n = 64
    pcm = bench.synth_pcm(n, seed=0)
    P = bench.unit_rows(100, 192, seed=1)
    E, Eb, re = eng.embed_pcm(torch.from_numpy(pcm).cuda())
    Pn, Pb, rp = eng.l2norm(torch.from_numpy(P).cuda())
    gidx, gsc = eng.affinity_topk(E, Eb, re, Pn, Pb, rp.max().reshape(1), k=1)
    torch.cuda.synchronize()
    model = oecapa.EcapaOracle(W.synthetic_weights(0), "fp32", torch.float64)
    Eo = oecapa.l2_normalise(model.embed(torch.from_numpy(ofbank.fbank(pcm))).numpy())
    rep = bench.parity_object(E.cpu().numpy(), gidx.cpu().numpy()[:, 0], gsc.cpu().numpy()[:, 0], Eo, P)
    print("\nprecise-mode parity vs the un-rounded oracle:", json.dumps(rep))
    assert rep["max_abs_dscore_all_pairs"] <= PRECISE_SCORE_BOUND and rep["max_abs_dscore_top1"] <= PRECISE_SCORE_BOUND
    assert rep["id_mismatches"] == 0
    assert rep["min_cos_embedding"] > 1 - 1e-11


def test_backend_in_precise_mode_end_to_end(tmp_path, monkeypatch):
    """SDK_PRECISION=1 through the plug-in API: enroll under the precise mode, identify under both - the two modes embed into the same
    space (scores differ at the 4e-3 level), so a vector enrolled in one is found by the other."""
    monkeypatch.setenv("SPEAKERS_EMBEDDINGS_DIR", str(tmp_path))
    wav, B = sub("wav"), sub("backend")
    t = np.arange(16000 * 6) / 16000.0
    rng = np.random.default_rng(1)
    x = sum((0.5 / h) * np.sin(2 * np.pi * 130.0 * h * t + rng.uniform(0, 6.28)) for h in range(1, 10)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.1 * t))
    wav.write_wav_s16(tmp_path / "a.wav", np.clip(np.round(x / np.abs(x).max() * 0.5 * 32767), -32768, 32767).astype(np.int16))
    monkeypatch.setenv("SDK_PRECISION", "1")
    be1 = B.Backend()
    rec = be1.enroll_speaker(tmp_path / "a.wav")
    cand = [{"id": "a", "embeddings": {"mi355x": [{"id": "emb-a", "external_id": rec["external_id"], "model_version": rec["model_version"]}]}}]
    rows1 = be1.identify_speaker(tmp_path / "a.wav", cand)
    assert be1.engine().precision == 1 and rows1 and rows1[0]["speaker_id"] == "a" and rows1[0]["similarity"] > 0.95
    # (every Backend owns its Engine; each call names its format - sdk_fbank_fmt, the blob descriptor - so the shared library context holds no per-engine state)
    monkeypatch.setenv("SDK_PRECISION", "0")
    be0 = B.Backend()
    assert be0.model_version == be1.model_version
    rows0 = be0.identify_speaker(tmp_path / "a.wav", cand)
    assert be0.engine().precision == 0 and rows0[0]["speaker_id"] == "a" and abs(rows0[0]["similarity"] - rows1[0]["similarity"]) < 2e-2
