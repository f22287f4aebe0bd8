"""GPU checks of the diarization's assignment stage (sdk_diarize_centroids, sdk_diarize_assign; Diarizer.run(constrained=True)) against the
all-maps float64 reference of tests/assign_ref.py.  Each test prints its figures before it asserts; the printed bounds and margins of a run
on an MI355X are recorded in profiles/r11_diarize_assign_parity.txt.

The kernel's arithmetic bound (test 6, used by 9): sdk_diarize_assign forms every cosine as d float64 fused multiply-adds in column order,
of unit rows, so a cosine is off the exact one by at most d 2^-53 (sum |e_j c_j| <= 1); the reference's own dot product by as much; a
chunk's total adds at most three cosines with two more roundings of a number below 3.  Two totals compared: 3 * 2 * d 2^-53 + 6 * 2^-52 =
(3 d + 6) 2^-52, the issue's "3 d 2^-52 in round figures".  score is an fp32 number, so it can equal the float64 reference cosine only to
that bound PLUS half an fp32 ulp of a number below 1 (2^-25)."""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assign_ref as AR  # noqa: E402
import diarize_ref as DR  # noqa: E402
import resnet_ref as RR  # noqa: E402

PKG = "speaker-diarization-toolkit_amd"
dz = importlib.import_module(f"{PKG}.diarize")
seg = importlib.import_module(f"{PKG}.segmentation")
rn = importlib.import_module(f"{PKG}.resnet")
cluster = importlib.import_module(f"{PKG}.cluster")
LIB = importlib.import_module(f"{PKG}._lib")
pytestmark = pytest.mark.gpu
F = 589
T4_CHUNK = 126
D = 192


def kernel_bound(d: int) -> float:
    return (3 * d + 6) * 2.0 ** -52


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_assign(engine, E, info, cent64, constrained):
    lab, sc = dz.diarize_assign(engine, dev(E), dev(info), dev(np.asarray(cent64, np.float64)), constrained)
    torch.cuda.synchronize()
    return lab.cpu().numpy(), sc.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 5: centroids
@pytest.mark.parametrize("K,Cn,d", [(1, 5, 192), (3, 40, 192), (40, 300, 192), (300, 50, 256)])
def test_centroids_against_float64(engine, K, Cn, d):
    """The float64 sums are taken in the reference's order, the division by the count is the same operation; only the order of the norm's
    sum of squares differs: the norm is off by at most (d + 2) 2^-53 relative, and cent64 by that plus one rounding of the last division.
    cent is cent64 rounded once, so it is within one fp32 ulp of the rounded reference."""
    E, info, train, tl = AR.make_case(40 + K, Cn, K, d=d)
    order = np.random.default_rng(K).permutation(K)                       # labels not sorted by row
    tl = order[tl].astype(np.int32)
    ref = AR.centroids(E, info, train, tl)
    cent, cent64 = dz.diarize_centroids(engine, dev(E), dev(train.astype(np.int32)), dev(tl), K)
    torch.cuda.synchronize()
    c32, c64 = cent.cpu().numpy(), cent64.cpu().numpy()
    e64 = float(np.abs(c64 - ref).max())
    bound64 = (d + 4) * 2.0 ** -53
    ulps = np.abs(c32.astype(np.float64) - ref.astype(np.float32).astype(np.float64)) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    print(f"centroids K={K} n={len(train)} d={d}: cent64 max|d| {e64:.3e} (bound {bound64:.3e}); cent vs fp32(reference): worst {ulps.max():.1f} ulp")
    assert np.isfinite(c64).all() and e64 <= bound64 and ulps.max() <= 1.0
    assert np.array_equal(c32, c64.astype(np.float32))
    # a cluster without rows gives a zero row; a second run is bit-identical
    cent2, cent64b = dz.diarize_centroids(engine, dev(E), dev(train.astype(np.int32)), dev(tl), K + 1)
    torch.cuda.synchronize()
    assert not cent2[K].any() and not cent64b[K].any() and torch.equal(cent64b[:K], cent64)


# ------------------------------------------------------------------------------------------------ 6: assignment, both modes
@pytest.mark.parametrize("K", [1, 2, 3, 40, 300])
@pytest.mark.parametrize("Cn", [1, 7, 3591])
def test_assign_equals_the_all_maps_reference(engine, Cn, K):
    E, info, train, tl = AR.make_case(1000 * K + Cn, Cn, K)
    cent = AR.centroids(E, info, train, tl)
    E, info = E[:3 * Cn], info[:Cn]                                      # the training chunks behind the Cn chunks have served
    bound = kernel_bound(D)
    for constrained in (False, True):
        ref = AR.assign(E, info, None, None, constrained=constrained, cent=cent)
        lab, sc = run_assign(engine, E, info, cent, constrained)
        least = float(ref["margin"].min())
        left_out = int((ref["margin"] <= bound).sum())
        err = float(np.abs(sc.astype(np.float64) - ref["score"]).max())
        print(f"assign C={Cn} K={K} constrained={int(constrained)}: bound {bound:.3e}; reference's least decisive margin {least:.3e} (must exceed "
              f"{10 * bound:.3e}); chunks left out {left_out}; chunks where the constraint bites {ref['bites'].mean():.3f}; candidates per chunk "
              f"{np.bincount(ref['m'], minlength=4).tolist()}; score max|d| {err:.3e} (bound {bound + 2.0 ** -25:.3e})")
        assert least > 10 * bound and left_out == 0
        assert ref["bites"].mean() >= 0.1
        assert np.array_equal(lab, ref["labels"])
        assert err <= bound + 2.0 ** -25 and not sc[ref["labels"] < 0].any()
        if constrained:
            nonneg = np.where(lab >= 0, lab, -1 - np.arange(3)[None, :])
            assert all(len(set(r)) == 3 for r in nonneg.tolist())                 # pairwise different within a chunk
        else:
            assert np.array_equal(lab >= 0, np.isfinite(E.reshape(Cn, 3, -1)).all(2))   # every candidate has a cluster


def test_assign_empty_and_wide_rows(engine):
    lab, sc = dz.diarize_assign(engine, torch.empty((0, D), device="cuda"), torch.empty((0, 3, 4), dtype=torch.int32, device="cuda"),
                                torch.zeros((2, D), dtype=torch.float64, device="cuda"), True)
    assert lab.shape == (0, 3) and sc.shape == (0, 3)
    E, info, train, tl = AR.make_case(77, 30, 5, d=256)
    cent = AR.centroids(E, info, train, tl)
    ref = AR.assign(E, info, None, None, cent=cent)
    lab, _ = run_assign(engine, E, info, cent, True)
    assert ref["margin"].min() > 10 * kernel_bound(256) and np.array_equal(lab, ref["labels"])


# ------------------------------------------------------------------------------------------------ 7: ties and K < m, bit for bit
def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def test_ties_and_fewer_centroids_bit_for_bit(engine):
    rng = np.random.default_rng(5)
    K = 4
    cen = unit(rng.standard_normal((K, D)))
    row = unit(cen[2] + 0.5 * cen[1] + 0.02 * rng.standard_normal(D))
    E = np.full((6, D), np.nan, np.float32)
    E[0] = E[2] = E[3] = E[4] = row                                      # chunk 0: slots 0 and 2; chunk 1: slots 0 and 1
    info = np.zeros((2, 3, 4), np.int32)
    info[0, 0] = info[0, 2] = info[1, 0] = info[1, 1] = (100, 50, 1, 1)
    cent = cen.astype(np.float64)
    ref = AR.assign(E, info, None, None, cent=cent)
    assert ref["labels"].tolist() == [[1, -1, 2], [1, 2, -1]] and ref["margin"].max() == 0.0       # two equal rows: a + b = b + a in any IEEE arithmetic
    outs = [run_assign(engine, E, info, cent, True) for _ in range(2)]
    assert outs[0][0].tolist() == [[1, -1, 2], [1, 2, -1]]
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert outs[0][1][0, 0] == outs[0][1][1, 0] and outs[0][1][0, 2] == outs[0][1][1, 1] and outs[0][1][0, 0] < outs[0][1][0, 2]
    assert run_assign(engine, E, info, cent, False)[0].tolist() == [[2, -1, 2], [2, 2, -1]]
    # one centroid, three candidates: the largest cosine keeps it, lowest slot on a tie
    near, far = unit(cen[0] + 0.3 * unit(rng.standard_normal(D))), unit(cen[0] + 0.9 * unit(rng.standard_normal(D)))
    for rows, want in (((near, far, near), [0, -1, -1]), ((far, near, near), [-1, 0, -1]), ((far, far, near), [-1, -1, 0])):
        E1 = np.stack(rows)
        info1 = np.zeros((1, 3, 4), np.int32)
        info1[0] = (100, 50, 1, 1)
        a, b = run_assign(engine, E1, info1, cent[:1], True), run_assign(engine, E1, info1, cent[:1], True)
        assert a[0][0].tolist() == want == AR.assign(E1, info1, None, None, cent=cent[:1])["labels"][0].tolist()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (a[1][0] != 0).sum() == 1
    # two centroids, three candidates: two get different clusters, one is dropped
    E2 = np.stack([near, unit(cen[1] + 0.5 * unit(rng.standard_normal(D))), far])
    ref2 = AR.assign(E2, info1, None, None, cent=cent[:2])
    got = run_assign(engine, E2, info1, cent[:2], True)[0]
    assert ref2["margin"][0] > 10 * kernel_bound(D) and np.array_equal(got, ref2["labels"]) and sorted(got[0].tolist()) == [-1, 0, 1]


# ------------------------------------------------------------------------------------------------ 8: end to end with a split chunk
RATE = 16000
FACTOR = 3.0


def voice(seed: int, lo: float, hi: float, am: float, n: int) -> np.ndarray:
    """A stand-in voice: seeded noise limited to the band lo .. hi Hz, gated on and off am times a second."""
    rng = np.random.default_rng(seed)
    X = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1 / RATE)
    X[(f < lo) | (f > hi)] = 0
    t = np.arange(n) / RATE
    x = np.fft.irfft(X, n) * (0.05 + 0.5 * (1 + np.tanh(4 * np.sin(2 * np.pi * am * t))))
    return x / np.abs(x).max() * 0.3


VOICES = [(101, 100.0, 700.0, 4.0), (202, 2500.0, 4000.0, 9.0), (303, 5000.0, 7500.0, 2.0)]
# (voice, from s, to s).  tests/test_diarize_gpu.py's layout has voice 0 return at 24 s, over voice 1; under the constrained rule the three
# chunks of that overlap have decisive margins of 0.003 - 0.009 in the CPU reference, below 10 x the row displacement (0.044), so here voice 0
# returns at 28 s, after voice 1 has ended (the overlap case stays with the older test, under the unconstrained rule).
LAYOUT = [(0, 2.0, 13.0), (1, 15.0, 27.0), (0, 28.0, 33.0), (2, 34.0, 41.0)]
N_SAMPLES = 42 * RATE
UNDERTONE = (1, 7.5, 13.0, 0.65)              # (voice, from s, to s, gain): voice 1, unseen by the class table, under the second half of voice 0's first turn
STEP_S = 2.5
E2E_THRESHOLD = 0.507        # the middle of the reference linkage's merge heights 0.446 and 0.568
E2E_MIN_CLUSTER = 2
SPLIT_CHUNK, SPLIT_KIND = 1, "halves"        # see split_chunk and the comment above the end-to-end test


def split_chunk(cls, c: int, kind: str):
    """The chunk c holds local speaker 0 alone (class 1): give part of its active frames to local speaker 1 (class 2).
    halves: the second half; tail: the last fifth; blocks: alternating blocks of 59 frames, the second of every pair."""
    on = np.flatnonzero(cls[c] == 1)
    assert len(on) and set(np.unique(cls[c])) <= {0, 1}
    if kind == "halves":
        move = on[len(on) // 2:]
    elif kind == "tail":
        move = on[-(len(on) // 5):]
    else:
        move = on[(np.arange(len(on)) // 59) % 2 == 1]
    out = cls.copy()
    out[c, move] = 2
    return out


def scenario(split=(SPLIT_CHUNK, SPLIT_KIND)):
    """-> (int16 recording, chunk starts, cls [C, 589]): local speakers of a chunk are numbered by first appearance in it."""
    x = np.random.default_rng(7).normal(0, 0.001, N_SAMPLES)
    for v, a, b in LAYOUT:
        i0, i1 = int(a * RATE), int(b * RATE)
        x[i0:i1] += voice(*VOICES[v], i1 - i0)
    v, a, b, gain = UNDERTONE
    i0, i1 = int(a * RATE), int(b * RATE)
    x[i0:i1] += gain * voice(*VOICES[v], i1 - i0)
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
    return pcm, st, (split_chunk(cls, *split) if split else cls)


def logp_of(cls):
    lp = np.full(cls.shape + (7,), -20.0, np.float32)
    np.put_along_axis(lp, cls[..., None].astype(np.int64), 0.0, axis=-1)
    return lp


def one_cos(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 1.0 - (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


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


def reference_pipeline(cls, st, E, info, constrained=True):
    """diarize_ref.pipeline with assign_ref's assignment: -> dict with the cut gap and the least decisive margin."""
    tr = DR.training(info, F)
    tl, Z = DR.cluster_training(np.asarray(E, np.float64)[tr], E2E_THRESHOLD, E2E_MIN_CLUSTER)
    a = AR.assign(E, info, tr, tl, constrained=constrained)
    K = a["centroids"].shape[0]
    labels, new, count, speakers, tn = DR.stitch(cls, st, a["labels"], K, N_SAMPLES)
    h = Z[:, 2]
    return dict(K=K, train=tr, labels=labels, raw_labels=a["labels"], centroids=a["centroids"][np.argsort(new)], count=count, speakers=speakers,
                turns=tn, cut_gap=float(np.abs(h - E2E_THRESHOLD).min()) if len(h) else np.inf, margin=float(a["margin"].min()),
                margins=a["margin"], bites=a["bites"])


# The split: chunk 1 (2.5 - 12.5 s) holds voice 0 alone; the second half of its active frames (halves) goes to local speaker 1.  Searched on
# the CPU reference: with the older test's scenario as it is, chunks 0 - 2 x (halves, a tail of a fifth, alternating blocks of 59 frames) give
# the split chunk a decisive margin of 0.0005 - 0.017: the two rows are the same voice, and giving them the two clusters one way round or the
# other costs nearly the same.  None reaches 10 x the row displacement (0.027 - 0.044, by the probe chunks).  So the scenario differs from
# that test's in two ways: no overlap (LAYOUT's comment), and UNDERTONE: voice 1 also sounds, at 0.65 of its level, under the second half of
# voice 0's first turn, without the class table knowing.  The two halves of the split chunk then differ in how far they lean to a second
# cluster, while one cluster stays the nearest of both (unconstrained: both rows in it, least margin 0.046), and the constrained optimum is
# decisive: the split chunk's margin is 0.061, the least over all chunks 0.048 (chunk 0), the cut gap 0.061, against 10 x the row displacement
# = 0.027.  Gains 0.15 - 0.85 were tried: below 0.6 and above 0.7 one of the figures falls under 0.044.  (The weights are synthetic: which
# cluster a voice lands in carries no meaning, only that the reference and the GPU agree.)  The test prints the figures;
# profiles/r11_diarize_assign_parity.txt records them.


@pytest.fixture(scope="module")
def weights():
    return rn.synthetic_weights(0)


def test_end_to_end_constrained_equals_the_reference(engine, weights):
    pcm, st, cls = scenario()
    E, info = reference_embeddings(weights, pcm, st, cls)
    ref = reference_pipeline(cls, st, E, info, True)
    free = reference_pipeline(cls, st, E, info, False)
    probe = [SPLIT_CHUNK, 9]
    e32, _ = reference_embeddings(weights, pcm, st, cls, acc=torch.float32, chunks=probe)
    ok = info[probe].reshape(-1, 4)[:, 3] != 0
    bound = FACTOR * float(one_cos(e32[ok], E.reshape(len(st), 3, -1)[probe].reshape(len(ok), -1)[ok]).max())
    move = float(np.sqrt(2 * bound))                                      # a unit row whose 1 - cos to the reference is `bound` has moved by sqrt(2 bound)
    flat = info.reshape(-1, 4)
    excluded = int(((flat[:, 0] > 0) & (flat[:, 3] == 0)).sum())
    c = SPLIT_CHUNK
    print(f"e2e constrained reference: K={ref['K']} train={len(ref['train'])} embedding bound (1 - cos) {bound:.3e} -> row displacement {move:.3e}; "
          f"cut gap {ref['cut_gap']:.3e}, least decisive margin {ref['margin']:.3e}, split chunk {c} ({SPLIT_KIND}) margin {ref['margins'][c]:.3e}, "
          f"unconstrained least margin {free['margin']:.3e} (each must exceed {10 * move:.3e}); excluded rows {excluded}; "
          f"split chunk labels: free {free['raw_labels'][c].tolist()} constrained {ref['raw_labels'][c].tolist()}; chunks where the constraint bites {int(ref['bites'].sum())}")
    assert ref["K"] == 3 and excluded == 0 and ref["bites"][c]
    assert ref["cut_gap"] > 10 * move and ref["margin"] > 10 * move and free["margin"] > 10 * move and move >= bound
    net = rn.ResNet34(engine, weights, precision=0)
    d = dz.Diarizer(engine, None, net)
    kw = dict(step_s=STEP_S, threshold=E2E_THRESHOLD, min_cluster_size=E2E_MIN_CLUSTER, logp=logp_of(cls))
    old = d.run(pcm, **kw)
    assert old.scores is None and np.array_equal(old.labels, free["labels"])
    assert old.labels[c, 0] == old.labels[c, 1] >= 0                     # today's rule: two local speakers of one chunk in one cluster
    res = d.run(pcm, constrained=True, **kw)
    print(f"e2e constrained gpu: K={res.n_speakers} split chunk labels {res.labels[c].tolist()} scores {res.scores[c].tolist()} "
          f"centroid 1 - cos vs reference {one_cos(res.centroids, ref['centroids'])}")
    assert np.array_equal(res.info, info) and np.array_equal(res.cls.cpu().numpy(), cls)
    assert res.labels[c, 0] != res.labels[c, 1] and min(res.labels[c, :2]) >= 0
    assert np.array_equal(res.labels, ref["labels"])
    assert np.array_equal(res.count, ref["count"]) and np.array_equal(res.speakers, ref["speakers"])
    assert res.turns == ref["turns"] and res.n_speakers == 3
    assert dz.to_rttm(res.turns, "rec") == DR.rttm(ref["turns"], "rec")
    assert res.scores.shape == (len(st), 3) and res.scores.dtype == np.float32 and not res.scores[res.labels < 0].any()


# ------------------------------------------------------------------------------------------------ 9: the model's own logp
def test_backend_diarize_constrained_with_the_models_own_logp(engine, monkeypatch):
    """Noise-like class tables.  Both sides read the GPU's own embeddings, so only the kernel's arithmetic bound separates sdk_diarize_assign
    from the host restatement; the margins of noise are not under the test's control, so chunks below 10 x the bound may be left out, at
    most 5 % of them.  On seeded unit rows of this shape (assign_ref.make_case, 3 591 chunks, on the CPU) the least margin is 5e-5,
    eight orders above the bound of 1.3e-13: the expected number left out is zero."""
    for k in ("SDK_MODEL", "SDK_NO_TORCH", "SDK_PRECISION", "SDK_RESNET_WEIGHTS", "SDK_SEGMENTATION_WEIGHTS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SDK_DIARIZE_BATCH", "5")
    be = importlib.import_module(f"{PKG}.backend").Backend()
    pcm, _, _ = scenario(None)
    pcm = pcm[:23 * RATE + 333]
    kw = dict(step_s=1.0, threshold=0.5, min_cluster_size=2)
    a = be.diarize(pcm, constrained=True, **kw)
    b = be.diarize(pcm, constrained=True, **kw)
    assert a.turns == b.turns and np.array_equal(a.labels, b.labels) and np.array_equal(a.scores, b.scores) and np.array_equal(a.centroids, b.centroids)
    Cn, K = len(a.starts), a.n_speakers
    assert a.labels.shape == (Cn, 3) and a.scores.shape == (Cn, 3) and np.isfinite(a.scores).all() and not a.scores[a.labels < 0].any()
    for row in a.labels.tolist():
        used = [k for k in row if k >= 0]
        assert len(set(used)) == len(used)
    # the GPU's own embeddings, batch by batch as Diarizer.run takes them
    dzr = be.diarizer()
    eng = dzr.eng
    prec = eng.precision
    eng.set_precision(dzr.resnet.precision)
    try:
        rec = torch.from_numpy(pcm).to(eng.device)
        sd = torch.from_numpy(a.starts.astype(np.int32)).to(eng.device)
        Es = [dzr.embed_chunks(rec, len(pcm), sd[i:i + 5])[2] for i in range(0, Cn, 5)]
        E_dev = torch.cat(Es)
        torch.cuda.synchronize()
    finally:
        eng.set_precision(prec)
    E = E_dev.cpu().numpy()
    train = dz.training_rows(a.info, F)
    tl = cluster.agglomerative_cluster(eng, E_dev.index_select(0, torch.from_numpy(train).to(eng.device)).contiguous(), 0.5, 2).labels if len(train) > 1 \
        else np.zeros(len(train), np.int32)
    host_labels, host_cent = dz.assign_constrained_host(E, a.info, train, tl)
    assert host_cent.shape == (K, D)
    ref = AR.assign(E, a.info, list(train), list(tl))
    bound = kernel_bound(D)
    keep = ref["margin"] > 10 * bound
    left_out = int((~keep).sum())
    finite = ref["margin"][np.isfinite(ref["margin"])]
    print(f"own logp constrained: {Cn} chunks, K={K}, {len(a.turns)} turns; bound {bound:.3e}; least decisive margin "
          f"{(finite.min() if len(finite) else np.inf):.3e}; chunks left out {left_out} of {Cn}; chunks where the constraint bites {int(ref['bites'].sum())}")
    assert left_out <= 0.05 * Cn
    if K:
        new = np.argmax(host_cent.astype(np.float64) @ a.centroids.astype(np.float64).T, axis=1)       # the renumbering by appearance
        assert sorted(new.tolist()) == list(range(K))
        mapped = np.where(host_labels >= 0, new[np.maximum(host_labels, 0)], -1)
        assert np.array_equal(mapped[keep], a.labels[keep])
        assert np.abs(host_cent[np.argsort(new)] - a.centroids).max() <= 2.0 ** -23
    count, speakers, _, _ = DR.reconstruct(a.cls.cpu().numpy(), a.starts, a.labels, max(K, 1), len(pcm))
    assert np.array_equal(a.count, count) and np.array_equal(a.speakers, speakers)
    assert be.diarize(np.zeros(0, np.int16), constrained=True).turns == []
    short = be.diarize(pcm[:5 * RATE], threshold=0.5, constrained=True)
    assert short.scores.shape == (1, 3) and len(short.starts) == 1


# ------------------------------------------------------------------------------------------------ 10: refusals
def test_refusals_are_python_exceptions(engine):
    E = torch.zeros((6, D), device="cuda")
    info = torch.ones((2, 3, 4), dtype=torch.int32, device="cuda")
    cent = torch.zeros((2, D), dtype=torch.float64, device="cuda")
    rows = torch.tensor([0, 3], dtype=torch.int32, device="cuda")
    labs = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="fp32"):
        dz.diarize_assign(engine, E.double(), info, cent, True)
    with pytest.raises(ValueError, match="fp32"):
        dz.diarize_assign(engine, E[0], info, cent, True)
    with pytest.raises(ValueError, match="info"):
        dz.diarize_assign(engine, E, info.long(), cent, True)
    with pytest.raises(ValueError, match="info"):
        dz.diarize_assign(engine, E, info[:1], cent, True)
    with pytest.raises(ValueError, match="float64"):
        dz.diarize_assign(engine, E, info, cent.float(), True)
    with pytest.raises(ValueError, match="float64"):
        dz.diarize_assign(engine, E, info, cent[:, :128], True)
    with pytest.raises(ValueError, match="K=0"):
        dz.diarize_assign(engine, E, info, cent[:0], True)
    with pytest.raises(ValueError, match="d=100 not supported"):
        dz.diarize_assign(engine, torch.zeros((6, 100), device="cuda"), info, torch.zeros((2, 100), dtype=torch.float64, device="cuda"), True)
    with pytest.raises(ValueError, match="d=576 not supported"):
        dz.diarize_centroids(engine, torch.zeros((6, 576), device="cuda"), rows, labs, 2)
    with pytest.raises(ValueError, match="K=0"):
        dz.diarize_centroids(engine, E, rows, labs, 0)
    with pytest.raises(ValueError, match="int32"):
        dz.diarize_centroids(engine, E, rows.long(), labs, 2)
    with pytest.raises(ValueError, match=r"rows must lie in \[0, 6\)"):
        dz.diarize_centroids(engine, E, rows + 4, labs, 2)
    st = torch.cuda.current_stream().cuda_stream
    lab = torch.empty((2, 3), dtype=torch.int32, device="cuda")
    sc = torch.empty((2, 3), device="cuda")
    lib = engine.lib
    with pytest.raises(LIB.SdkError, match="d=100 not supported"):
        LIB.check(lib.sdk_diarize_assign(engine.ctx, E.data_ptr(), info.data_ptr(), cent.data_ptr(), 2, 2, 100, 1, lab.data_ptr(), sc.data_ptr(), st), "sdk_diarize_assign")
    with pytest.raises(LIB.SdkError, match="K=0"):
        LIB.check(lib.sdk_diarize_assign(engine.ctx, E.data_ptr(), info.data_ptr(), cent.data_ptr(), 2, 0, D, 1, lab.data_ptr(), sc.data_ptr(), st), "sdk_diarize_assign")
    with pytest.raises(LIB.SdkError, match="constrained=2"):
        LIB.check(lib.sdk_diarize_assign(engine.ctx, E.data_ptr(), info.data_ptr(), cent.data_ptr(), 2, 2, D, 2, lab.data_ptr(), sc.data_ptr(), st), "sdk_diarize_assign")
    with pytest.raises(LIB.SdkError, match="null argument"):
        LIB.check(lib.sdk_diarize_assign(engine.ctx, E.data_ptr(), None, cent.data_ptr(), 2, 2, D, 1, lab.data_ptr(), sc.data_ptr(), st), "sdk_diarize_assign")
    with pytest.raises(LIB.SdkError, match="K=0"):
        LIB.check(lib.sdk_diarize_centroids(engine.ctx, E.data_ptr(), rows.data_ptr(), labs.data_ptr(), 2, 0, D, cent.data_ptr(), None, st), "sdk_diarize_centroids")
    l2, s2 = dz.diarize_assign(engine, E, info, cent, True)               # the device is fine after the refusals
    torch.cuda.synchronize()
    assert l2.shape == (2, 3) and torch.isfinite(s2).all()
