"""GPU checks of the diarization pipeline: the integer kernels (csrc/diarize.hip) bit for bit against tests/diarize_ref.py, the masked pooling
and the masked ResNet34 forward against float64 within 3x the deviation of an fp32 restatement (the project's convention for every family;
the yardsticks are measured on the CPU inside each test and recorded in profiles/r10_diarize_parity.txt), and the whole pipeline against the
CPU reference pipeline.  Each test prints its figures before it asserts."""
from __future__ import annotations

import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diarize_ref as DR  # noqa: E402
import resnet_ref as RR  # noqa: E402

PKG = "speaker-diarization-toolkit_amd"
dz = importlib.import_module(f"{PKG}.diarize")
seg = importlib.import_module(f"{PKG}.segmentation")
rn = importlib.import_module(f"{PKG}.resnet")
LIB = importlib.import_module(f"{PKG}._lib")
pytestmark = pytest.mark.gpu
BITS = {0: 8, 2: 11}
DT = {0: torch.bfloat16, 2: torch.float16}
FACTOR = 3.0
F = 589
T_CHUNK, T4_CHUNK = 1001, 126


@pytest.fixture(scope="module")
def weights():
    return rn.synthetic_weights(0)


@pytest.fixture(scope="module")
def nets(engine, weights):
    return {p: rn.ResNet34(engine, weights, precision=p) for p in (0, 2)}


def random_cls(rng, Cn, p_sil=0.3):
    cls = np.zeros((Cn, F), np.uint8)
    for c in range(Cn):
        i = 0
        while i < F:
            n = int(rng.integers(1, 90))
            cls[c, i:i + n] = 0 if rng.random() < p_sil else rng.integers(1, 7)
            i += n
    return cls


def one_cos(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 1.0 - (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


# ------------------------------------------------------------------------------------------------ (a), (b), (d): bit for bit
def test_decode_and_masks_bit_for_bit(engine):
    rng = np.random.default_rng(0)
    for Cn in (1, 37):
        logp = rng.standard_normal((Cn, F, 7)).astype(np.float32)
        logp[0, :40, 1] = logp[0, :40, 4] = 7.0                          # ties: the lower class
        logp[0, 40:60] = -1.5                                            # all equal: class 0
        cls = dz.powerset_decode(engine, torch.from_numpy(logp).cuda())
        torch.cuda.synchronize()
        assert np.array_equal(cls.cpu().numpy(), DR.decode(logp))
    cls = random_cls(rng, 9)
    cls[3] = 5
    cls[4, 7:] = 0
    cls[5] = 0
    for T4 in (126, 26, 1):
        w, info = dz.diarize_masks(engine, torch.from_numpy(cls).cuda(), T4)
        torch.cuda.synchronize()
        rw, rinfo = DR.masks(cls, T4)
        assert np.array_equal(w.cpu().numpy(), rw) and np.array_equal(info.cpu().numpy(), rinfo)


@pytest.mark.parametrize("step_s,n_s,K,maxsp,none", [(1.0, 10.0, 3, None, False), (1.0, 7.3, 2, None, False), (0.5, 21.4, 1, None, False),
                                                     (2.5, 47.9, 70, None, False), (1.0, 33.3, 6, 1, False), (1.0, 19.0, 4, None, True),
                                                     (2.5, 23.0, 5, 0, False)])
def test_reconstruct_bit_for_bit(engine, step_s, n_s, K, maxsp, none):
    """C = 1 (10 s and 7.3 s), steps 0.5 s and 2.5 s, K = 1 and K = 70, labels all -1, max_speakers 1 and 0."""
    n = int(n_s * 16000) + (131 if n_s != 10.0 else 0)
    st = seg.chunk_starts(n, step_s)
    assert (len(st) == 1) == (n_s <= 10.0)
    rng = np.random.default_rng(int(n_s * 10) + K)
    cls = random_cls(rng, len(st))
    labels = np.full((len(st), 3), -1, np.int32) if none else rng.integers(-1, K, (len(st), 3)).astype(np.int32)
    count, speakers, act = dz.diarize_reconstruct(engine, torch.from_numpy(cls).cuda(), torch.from_numpy(st.astype(np.int32)).cuda(),
                                                  torch.from_numpy(labels).cuda(), K, n, maxsp, want_act=True)
    torch.cuda.synchronize()
    rcount, rspeakers, ract, _ = DR.reconstruct(cls, st, labels, K, n, maxsp)
    assert np.array_equal(act.cpu().numpy(), ract)
    assert np.array_equal(count.cpu().numpy(), rcount) and np.array_equal(speakers.cpu().numpy(), rspeakers)


# ------------------------------------------------------------------------------------------------ masked pooling, kernel level
def masked_pool(engine, x, w, valid, prec):
    """x [B, F4, T4, C] 2-byte (device), w [B, S, T4], valid [B, S] -> [B, S, 2 C F4] fp32."""
    B, F4, T4, Cc = x.shape
    S = w.shape[1]
    out = torch.empty((B, S, 2 * Cc * F4), dtype=torch.float32, device="cuda")
    LIB.check(engine.lib.sdk_resnet_masked_pool(engine.ctx, x.data_ptr(), B, F4, T4, Cc, S, w.data_ptr(), valid.data_ptr(), out.data_ptr(), prec,
                                                torch.cuda.current_stream().cuda_stream), "sdk_resnet_masked_pool")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("kind", ["binary", "fractional"])
def test_masked_pooling_against_float64(engine, prec, kind):
    rng = np.random.default_rng(11 + prec)
    B, F4, T4, Cc, S = 3, 10, 126, 256, 3
    x = torch.from_numpy(np.abs(rng.standard_normal((B, F4, T4, Cc))).astype(np.float32) * 2).to(DT[prec])
    if kind == "binary":
        w = torch.from_numpy((rng.random((B, S, T4)) < 0.4).astype(np.float32))
        w[0, 1] = 0
        w[0, 1, 5] = w[0, 1, 90] = 1                                     # exactly two columns
    else:
        w = torch.from_numpy(rng.random((B, S, T4)).astype(np.float32))
    valid = torch.ones((B, S), dtype=torch.int32)
    last = x.float().permute(0, 3, 1, 2)                                 # [B, C, F4, T4], feature c F4 + f
    want = DR.weighted_stats(last, w)
    spread = float((DR.weighted_stats_fp32_in_order(last, w).double() - want).abs().max())
    got = masked_pool(engine, x.cuda(), w.cuda(), valid.cuda(), prec)
    err = float((got.double() - want).abs().max())
    print(f"masked pooling prec={prec} {kind}: fp32-in-order deviation {spread:.3e} bound {FACTOR * spread:.3e} gpu max|d| {err:.3e}")
    assert np.isfinite(err) and err <= FACTOR * spread
    if kind == "binary":                                                 # 0 / 1 weights: the unbiased statistic over the selected columns
        sel = w[2, 0].bool()
        ref = RR.tstp_stats(x[2:3, :, sel, :].float())
        assert float((got[2, 0].double() - ref[0]).abs().max()) <= FACTOR * spread


# ------------------------------------------------------------------------------------------------ the whole masked forward
def chunk_feats(engine, prec, B, seed):
    """B seeded 10-s chunks -> fbank features of the engine in precision prec: (device [B T, ldf], host float [B, T, 80])."""
    rng = np.random.default_rng(seed)
    t = np.arange(160000) / 16000.0
    pcm = np.stack([rng.normal(0, 0.08, 160000) * (1 + 0.5 * np.sin(2 * np.pi * (0.7 + b) * t)) + 0.2 * np.sin(2 * np.pi * (150.0 + 90 * b) * t)
                    for b in range(B)])
    pcm = np.clip(np.round(pcm * 32768), -32768, 32767).astype(np.int16)
    old = engine.precision
    engine.set_precision(prec)
    try:
        feats = engine.fbank(torch.from_numpy(pcm).cuda())
        torch.cuda.synchronize()
    finally:
        engine.set_precision(old)
    return feats, feats.float().cpu().reshape(B, -1, feats.shape[1])[:, :, :80]


@pytest.mark.parametrize("prec", [0, 2])
def test_masked_forward_against_the_layer_boundary_model(engine, nets, weights, prec):
    B, S = 2, 3
    feats, fh = chunk_feats(engine, prec, B, 5)
    assert fh.shape[1] == T_CHUNK and nets[prec].last_map_frames(T_CHUNK) == T4_CHUNK
    rng = np.random.default_rng(3)
    cls = random_cls(rng, B, 0.2)
    w, info = dz.diarize_masks(engine, torch.from_numpy(cls).cuda(), T4_CHUNK)
    valid = info[:, :, 3].contiguous()
    assert int(valid.sum()) >= 4
    got = nets[prec].forward_masked(feats, B, T_CHUNK, w, valid)
    got2 = nets[prec].forward_masked(feats, B, T_CHUNK, w, valid)
    torch.cuda.synchronize()
    assert torch.equal(got, got2), "two runs differ"
    got = got.cpu().numpy().reshape(B, S, -1)
    wh = w.cpu()
    e64 = DR.weighted_embed(weights, DR.last_map(weights, fh, BITS[prec], acc=torch.float64), wh).numpy()
    e32 = DR.weighted_embed(weights, DR.last_map(weights, fh, BITS[prec], acc=torch.float32), wh).numpy()
    ok = valid.cpu().numpy().astype(bool)
    spread = float(one_cos(e32, e64)[ok].max())
    err = float(one_cos(got, e64)[ok].max())
    print(f"masked forward prec={prec} T={T_CHUNK}: model fp32-vs-float64 spread (1 - cos) {spread:.3e} bound {FACTOR * spread:.3e} gpu {err:.3e}")
    assert np.isfinite(err) and err <= FACTOR * spread
    assert not got[~ok].any(), "valid = 0 rows must be zeros"


@pytest.mark.parametrize("prec", [0, 2])
def test_masked_forward_consistency(engine, nets, prec):
    B, S = 2, 3
    feats, _ = chunk_feats(engine, prec, B, 9)
    net = nets[prec]
    ones = torch.ones((B, 1, T4_CHUNK), dtype=torch.float32, device="cuda")
    v1 = torch.ones((B, 1), dtype=torch.int32, device="cuda")
    a = net.forward_masked(feats, B, T_CHUNK, ones, v1).cpu().numpy()
    b = net.forward(feats, B, T_CHUNK).cpu().numpy()
    # all-ones weights against sdk_resnet_forward: the same trunk and the same sums; only the mean's last step differs (s / v1 against
    # s * (1 / T)).  The pooling bound of the kernel-level test is a few 1e-7 absolute on statistics of order 1, i.e. <= 3e-6 relative; 1 - cos
    # is quadratic in a row's relative displacement, so with a factor 3 for seg_1's conditioning the bound is (3 * 3e-6)^2 ~ 1e-10
    d = float(one_cos(a, b).max())
    print(f"all-ones weights vs sdk_resnet_forward prec={prec}: 1 - cos {d:.3e}")
    assert d <= 1e-10
    rng = np.random.default_rng(2)
    w = torch.from_numpy(rng.random((B, S, T4_CHUNK)).astype(np.float32)).cuda()
    valid = torch.tensor([[1, 1, 1], [1, 0, 1]], dtype=torch.int32, device="cuda")
    e1 = net.forward_masked(feats, B, T_CHUNK, w, valid)
    w2 = w.clone()
    w2[:, 0] = torch.from_numpy(rng.random((B, T4_CHUNK)).astype(np.float32)).cuda()
    w2[:, 2] = 1.0
    e2 = net.forward_masked(feats, B, T_CHUNK, w2, valid)
    torch.cuda.synchronize()
    e1, e2 = e1.reshape(B, S, -1), e2.reshape(B, S, -1)
    assert torch.equal(e1[:, 1], e2[:, 1]), "speaker 1's rows changed with the other speakers' weights"
    assert not torch.equal(e1[:, 0], e2[:, 0])
    assert not e1[1, 1].any() and e1[0, 1].any()


# ------------------------------------------------------------------------------------------------ end to end
RATE = 16000


def voice(seed: int, lo: float, hi: float, am: float, n: int) -> np.ndarray:
    """A stand-in voice: seeded noise limited to the band lo .. hi Hz, gated on and off am times a second (syllable-like: the per-chunk mean
    normalisation of the fbank removes whatever is stationary, so the voices differ in band AND rhythm)."""
    rng = np.random.default_rng(seed)
    X = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1 / RATE)
    X[(f < lo) | (f > hi)] = 0
    t = np.arange(n) / RATE
    x = np.fft.irfft(X, n) * (0.05 + 0.5 * (1 + np.tanh(4 * np.sin(2 * np.pi * am * t))))
    return x / np.abs(x).max() * 0.3


VOICES = [(101, 100.0, 700.0, 4.0), (202, 2500.0, 4000.0, 9.0), (303, 5000.0, 7500.0, 2.0)]
LAYOUT = [(0, 2.0, 13.0), (1, 15.0, 27.0), (0, 24.0, 33.0), (2, 34.0, 41.0)]     # (voice, from s, to s): pause 13 - 15, overlap 24 - 27
N_SAMPLES = 42 * RATE
STEP_S = 2.5
E2E_THRESHOLD = 0.5          # between two merge heights of the reference's linkage that lie 0.13 apart (synthetic weights: chosen on the CPU reference)
E2E_MIN_CLUSTER = 2


def scenario():
    """-> (int16 recording, chunk starts, cls [C, 589]): local speakers of a chunk are numbered by first appearance in it."""
    x = np.random.default_rng(7).normal(0, 0.001, N_SAMPLES)
    for v, a, b in LAYOUT:
        i0, i1 = int(a * RATE), int(b * RATE)
        x[i0:i1] += voice(*VOICES[v], i1 - i0)
    pcm = np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)
    st = seg.chunk_starts(N_SAMPLES, STEP_S)
    cls = np.zeros((len(st), F), np.uint8)
    single = {0: 1, 1: 2, 2: 3}
    pair = {frozenset((0, 1)): 4, frozenset((0, 2)): 5, frozenset((1, 2)): 6}
    for c in range(len(st)):
        local = {}
        for i in range(F):
            t = (int(st[c]) + 270 * i + 495) / RATE
            on = sorted({v for v, a, b in LAYOUT if a <= t < b})
            for v in on:
                local.setdefault(v, len(local))
            ids = {local[v] for v in on}
            cls[c, i] = 0 if not ids else single[next(iter(ids))] if len(ids) == 1 else pair[frozenset(ids)]
        assert len(local) <= 3
    return pcm, st, cls


def logp_of(cls):
    lp = np.full(cls.shape + (7,), -20.0, np.float32)
    np.put_along_axis(lp, cls[..., None].astype(np.int64), 0.0, axis=-1)
    return lp


def reference_embeddings(weights, pcm, st, cls, bits=8, acc=torch.float64, chunks=None):
    """The CPU reference's unit embeddings [C * 3, d] (zeros where not valid) and info: oracle fbank, layer-boundary model, float64 pooling."""
    from oracle import fbank as ofbank
    w, info = DR.masks(cls, T4_CHUNK)
    E = []
    for c in (range(len(st)) if chunks is None else chunks):
        s = int(st[c])
        x = np.pad(pcm[s:s + 160000], (0, max(0, s + 160000 - len(pcm))))
        feats = RR.round_bits(torch.from_numpy(ofbank.fbank(x[None])).float(), bits)
        E.append(DR.weighted_embed(weights, DR.last_map(weights, feats, bits, acc=acc), torch.from_numpy(w[c:c + 1]))[0].numpy())
    E = np.concatenate(E)
    ok = (info if chunks is None else info[list(chunks)]).reshape(-1, 4)[:, 3] != 0
    E[~ok] = 0
    E[ok] /= np.linalg.norm(E[ok], axis=1, keepdims=True)
    return E, info


def decisive_margins(ref, threshold):
    """(gap of the cut to the nearest merge height, least best-minus-second cosine of an assignment) of a reference pipeline result."""
    h = ref["Z"][:, 2]
    return float(np.abs(h - threshold).min()) if len(h) else np.inf, float(min(ref["margins"])) if len(ref["margins"]) else np.inf


def test_end_to_end_with_injected_logp_equals_the_reference_turns(engine, nets, weights):
    pcm, st, cls = scenario()
    E, info = reference_embeddings(weights, pcm, st, cls)
    ref = DR.pipeline(cls, st, E, info, N_SAMPLES, E2E_THRESHOLD, E2E_MIN_CLUSTER)
    # the embedding bound at this T: 3 x the layer-boundary model's own fp32-vs-float64 spread, here on two chunks of this scenario
    probe = [2, 9]
    e32, _ = reference_embeddings(weights, pcm, st, cls, acc=torch.float32, chunks=probe)
    ok = info[probe].reshape(-1, 4)[:, 3] != 0
    bound = FACTOR * float(one_cos(e32[ok], E.reshape(len(st), 3, -1)[probe].reshape(len(ok), -1)[ok]).max())
    # a unit row whose 1 - cos to the reference is `bound` has moved by sqrt(2 bound): heights and cosines move by at most that per row
    move = float(np.sqrt(2 * bound))
    cut_gap, cos_gap = decisive_margins(ref, E2E_THRESHOLD)
    flat = info.reshape(-1, 4)
    excluded = int(((flat[:, 0] > 0) & (flat[:, 3] == 0)).sum())
    print(f"e2e reference: K={ref['K']} train={len(ref['train'])} embedding bound (1 - cos) {bound:.3e} -> row displacement {move:.3e}; "
          f"cut gap {cut_gap:.3e} assignment gap {cos_gap:.3e} (each must exceed {10 * move:.3e} >= 10 x the bound); excluded rows {excluded}")
    assert ref["K"] == 3 and excluded == 0
    assert cut_gap > 10 * move and cos_gap > 10 * move and move >= bound
    res = dz.Diarizer(engine, None, nets[0]).run(pcm, step_s=STEP_S, threshold=E2E_THRESHOLD, min_cluster_size=E2E_MIN_CLUSTER, logp=logp_of(cls))
    print(f"e2e gpu: K={res.n_speakers} centroid 1 - cos vs reference {one_cos(res.centroids, ref['centroids'])}")
    assert np.array_equal(res.cls.cpu().numpy(), cls)
    assert np.array_equal(res.info, info)
    assert np.array_equal(res.labels, ref["labels"])
    assert np.array_equal(res.count, ref["count"]) and np.array_equal(res.speakers, ref["speakers"])
    assert res.turns == ref["turns"] and res.n_speakers == 3
    assert dz.to_rttm(res.turns, "rec") == DR.rttm(ref["turns"], "rec")


def test_backend_diarize_with_the_models_own_logp(engine, monkeypatch):
    """Synthetic weights: the segmentation output is noise.  The call runs, is deterministic, and equals the reference's stitching fed with
    the GPU's own class table and labels."""
    for k in ("SDK_MODEL", "SDK_NO_TORCH", "SDK_PRECISION", "SDK_RESNET_WEIGHTS", "SDK_SEGMENTATION_WEIGHTS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SDK_DIARIZE_BATCH", "5")
    be = importlib.import_module(f"{PKG}.backend").Backend()
    pcm, _, _ = scenario()
    pcm = pcm[:23 * RATE + 333]
    a = be.diarize(pcm, step_s=1.0, threshold=0.5, min_cluster_size=2)
    b = be.diarize(pcm, step_s=1.0, threshold=0.5, min_cluster_size=2)
    assert a.turns == b.turns and np.array_equal(a.labels, b.labels) and np.array_equal(a.speakers, b.speakers) and np.array_equal(a.centroids, b.centroids)
    cls = a.cls.cpu().numpy()
    assert cls.shape == (len(seg.chunk_starts(len(pcm), 1.0)), F) and np.array_equal(a.info, DR.masks(cls, T4_CHUNK)[1])
    K = a.n_speakers
    count, speakers, _, _ = DR.reconstruct(cls, a.starts, a.labels, max(K, 1), len(pcm))
    assert np.array_equal(a.count, count) and np.array_equal(a.speakers, speakers)
    assert a.turns == DR.turns(speakers, K) and a.centroids.shape == (K, 192)
    if K:
        assert np.allclose(np.linalg.norm(a.centroids, axis=1), 1.0, atol=1e-5)
        assert DR.order_by_appearance(speakers, K) == list(range(K))
    print(f"own logp: {len(a.starts)} chunks, K={K}, {len(a.turns)} turns")
    short = be.diarize(pcm[:5 * RATE], threshold=0.5)
    assert short.count.shape == (dz.global_frames(5 * RATE),) and len(short.starts) == 1
    assert be.diarize(np.zeros(0, np.int16)).turns == []


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_are_python_exceptions(engine, nets, weights):
    net = nets[0]
    B = 1
    feats, _ = chunk_feats(engine, 0, B, 1)
    w = torch.ones((B, 3, T4_CHUNK), dtype=torch.float32, device="cuda")
    valid = torch.ones((B, 3), dtype=torch.int32, device="cuda")
    emb = torch.empty((3, 192), dtype=torch.float32, device="cuda")
    need = engine.lib.sdk_resnet_masked_workspace_bytes(C.byref(net.desc), B, T_CHUNK, 3)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(desc, nbytes):
        LIB.check(engine.lib.sdk_resnet_forward_masked(engine.ctx, net.blob.data_ptr(), C.byref(desc), feats.data_ptr(), feats.stride(0), B, T_CHUNK, 3,
                                                       w.data_ptr(), valid.data_ptr(), ws.data_ptr(), nbytes, emb.data_ptr(), st), "sdk_resnet_forward_masked")
    with pytest.raises(LIB.SdkError, match=rf"workspace of {need - 256} bytes, {need} needed"):
        call(net.desc, need - 256)
    d1 = rn.ResNetDesc.from_buffer_copy(net.desc)
    d1.precision = 1
    with pytest.raises(LIB.SdkError, match="precision 1 .* not built for the ResNet34 family"):
        call(d1, need)
    assert engine.lib.sdk_resnet_masked_workspace_bytes(C.byref(net.desc), B, T_CHUNK, 0) == 0
    with pytest.raises(ValueError, match="SDK_PRECISION=1"):
        rn.ResNet34(engine, weights, precision=1)
    n = 160000 + 160 * 21846
    with pytest.raises(ValueError, match=r"65536 rows .*step_s"):
        dz.Diarizer(engine, None, net).run(np.zeros(n, np.int16), step_s=0.01)
    call(net.desc, need)                                                 # the device is fine after the refusals
    torch.cuda.synchronize()
    assert torch.isfinite(emb).all()
    env = dict(os.environ, SDK_NO_TORCH="1")
    code = (f"import importlib, numpy as np\nbe = importlib.import_module('{PKG}.backend').Backend()\n"
            "try:\n    be.diarize(np.zeros(16000, np.int16))\nexcept ValueError as e:\n    print('REFUSED:', e)\n")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert "REFUSED: diarize needs the torch engine: not available with SDK_NO_TORCH=1" in out.stdout, out.stdout + out.stderr
