"""GPU checks of the speaker-count bounds (`speakers=` of Diarizer.run / run_many, Backend.cluster_ranges) on 30 - 42 s recordings at
step_s = 1 with an injected logp and synthetic weights, built as tests/test_diarize_assign_gpu.py builds its scenario.  The forced labels
are compared with the host pipeline of tests/diarize_ref.py extended in tests/kmeans_ref.py (level search, k-means), run on the GPU's own
embeddings, under the margin treatment of test_backend_diarize_constrained_with_the_models_own_logp: chunks whose decisive margin is at or
under 10 x the assignment kernel's bound may be left out, at most 5 % of them.  Each test prints its figures before it asserts."""
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
import kmeans_ref as KR  # noqa: E402

PKG = "speaker-diarization-toolkit_amd"
dz = importlib.import_module(f"{PKG}.diarize")
seg = importlib.import_module(f"{PKG}.segmentation")
rn = importlib.import_module(f"{PKG}.resnet")
cluster = importlib.import_module(f"{PKG}.cluster")
pytestmark = pytest.mark.gpu
F, RATE, D = 589, 16000, 192
VOICES = [(101, 100.0, 700.0, 4.0), (202, 2500.0, 4000.0, 9.0), (303, 5000.0, 7500.0, 2.0)]
LAYOUT = [(0, 2.0, 13.0), (1, 15.0, 27.0), (0, 28.0, 33.0), (2, 34.0, 41.0)]      # (voice, from s, to s): no overlap
THRESHOLD = {"ahc": 0.5, "vbx": cluster.VBX_AHC_THRESHOLD}
MIN_CLUSTER = 2


def voice(seed: int, lo: float, hi: float, am: float, n: int) -> np.ndarray:
    """A stand-in voice: seeded noise limited to the band lo .. hi Hz, gated on and off am times a second."""
    rng = np.random.default_rng(seed)
    X = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1 / RATE)
    X[(f < lo) | (f > hi)] = 0
    t = np.arange(n) / RATE
    x = np.fft.irfft(X, n) * (0.05 + 0.5 * (1 + np.tanh(4 * np.sin(2 * np.pi * am * t))))
    return x / np.abs(x).max() * 0.3


def recording(seconds: float):
    """-> (int16 samples, logp [C, 589, 7]) at step_s = 1: the class table says who of LAYOUT speaks, local speakers by first appearance."""
    n = int(seconds * RATE)
    x = np.random.default_rng(7).normal(0, 0.001, 42 * RATE)
    for v, a, b in LAYOUT:
        x[int(a * RATE):int(b * RATE)] += voice(*VOICES[v], int(b * RATE) - int(a * RATE))
    pcm = np.clip(np.round(x[:n] * 32768), -32768, 32767).astype(np.int16)
    st = seg.chunk_starts(n, 1.0)
    t = (st[:, None] + 270 * np.arange(F)[None, :] + 495) / RATE                  # [C, F] frame centres, s
    who = np.full(t.shape, -1)
    for v, a, b in LAYOUT:
        who[(t >= a) & (t < b) & (t < seconds)] = v
    cls = np.zeros(t.shape, np.uint8)
    for c in range(len(st)):
        local = {}
        for v in who[c][who[c] >= 0]:
            local.setdefault(int(v), len(local))
        for v, s in local.items():
            cls[c][who[c] == v] = s + 1
    lp = np.full(cls.shape + (7,), -20.0, np.float32)
    np.put_along_axis(lp, cls[..., None].astype(np.int64), 0.0, axis=-1)
    return pcm, lp


@pytest.fixture(scope="module")
def diarizer(engine):
    return dz.Diarizer(engine, None, rn.ResNet34(engine, rn.synthetic_weights(0), precision=0))


@pytest.fixture(scope="module")
def rec42():
    return recording(42.0)


_base = {}


def base_run(diarizer, rec42, clustering, constrained):
    """The unbounded result, once per (clustering, constrained)."""
    key = (clustering, constrained)
    if key not in _base:
        _base[key] = diarizer.run(rec42[0], logp=rec42[1], threshold=THRESHOLD[clustering], min_cluster_size=MIN_CLUSTER, clustering=clustering,
                                  constrained=constrained)
    return _base[key]


def same_result(a, b, scores=True) -> bool:
    """scores=False (run against run_many): scores and centroids to fp32 rounding of the same float64 rows, "shared" in diarize.py."""
    ok = (np.array_equal(a.labels, b.labels) and np.array_equal(a.count, b.count) and np.array_equal(a.speakers, b.speakers) and a.turns == b.turns
          and a.n_speakers == b.n_speakers and a.centroids.shape == b.centroids.shape)
    ok = ok and (np.array_equal(a.centroids, b.centroids) if scores else bool(np.abs(a.centroids - b.centroids).max(initial=0) <= 2.0 ** -23))
    if scores:
        ok = ok and ((a.scores is None and b.scores is None) or np.array_equal(a.scores, b.scores))
    return ok


# ------------------------------------------------------------------------------------------------ unbounded
@pytest.mark.parametrize("clustering", ["ahc", "vbx"])
@pytest.mark.parametrize("constrained", [False, True])
def test_inside_the_bounds_nothing_changes(diarizer, rec42, clustering, constrained):
    base = base_run(diarizer, rec42, clustering, constrained)
    K0 = base.n_speakers
    kw = dict(logp=rec42[1], threshold=THRESHOLD[clustering], min_cluster_size=MIN_CLUSTER, clustering=clustering, constrained=constrained)
    print(f"unbounded {clustering} constrained={int(constrained)}: K0 = {K0}, {len(base.turns)} turns")
    assert K0 >= 1 and base.forced is None
    for sp in (None, (max(K0 - 1, 1), K0 + 1), K0, (None, K0), (K0, None), (None, None)):
        res = diarizer.run(rec42[0], speakers=sp, **kw)
        assert same_result(base, res) and res.forced is None
        if clustering == "vbx":
            assert np.array_equal(res.pi, base.pi) and np.array_equal(res.elbo, base.elbo)


# ------------------------------------------------------------------------------------------------ forced, against the host pipeline
def own_embeddings(diarizer, pcm, logp):
    eng = diarizer.eng
    st = seg.chunk_starts(len(pcm), 1.0)
    rec = torch.from_numpy(pcm).to(eng.device)
    sd = torch.from_numpy(st.astype(np.int32)).to(eng.device)
    cls, info, E = diarizer._embed_all(rec, len(pcm), sd, torch.as_tensor(logp).to(eng.device))
    torch.cuda.synchronize()
    return st, cls.cpu().numpy(), info.cpu().numpy(), E.cpu().numpy()


@pytest.mark.parametrize("clustering", ["ahc", "vbx"])
def test_forced_counts_equal_the_host_pipeline(diarizer, rec42, clustering):
    from scipy.cluster.hierarchy import linkage
    pcm, logp = rec42
    base = base_run(diarizer, rec42, clustering, True)
    K0 = base.n_speakers
    st, cls, info, E = own_embeddings(diarizer, pcm, logp)
    assert np.array_equal(info, base.info)
    tr = np.asarray(DR.training(info, F))
    Et = E[tr].astype(np.float64)
    Z = linkage(Et, "centroid")
    bound = (3 * D + 6) * 2.0 ** -52                                      # test_diarize_assign_gpu.kernel_bound
    kw = dict(logp=logp, threshold=THRESHOLD[clustering], min_cluster_size=MIN_CLUSTER, clustering=clustering, constrained=True)
    for k in sorted({1, 2, K0 + 1}):
        res = diarizer.run(pcm, speakers=k, **kw)
        if k == K0:
            assert res.forced is None and same_result(base, res)
            continue
        if clustering == "ahc":
            tl, forced = KR.ahc_bounded(Z, Et, THRESHOLD["ahc"], MIN_CLUSTER, k, k)
            reachable, method = forced["reachable"], "level"
            assert res.forced == {q: forced[q] for q in ("found", "target", "method", "level", "n_iter")}
        else:
            km = KR.kmeans(E, k, rows=tr)
            kb = (3 * D + 5) * 2.0 ** -52                                 # test_kmeans_gpu.kmeans_bound
            print(f"forced vbx k={k}: k-means restatement's least margin over {km['n_iter']} iterations {km['least']:.3e} (must exceed {10 * kb:.3e})")
            assert km["least"] > 10 * kb
            tl, reachable, method = km["labels"], km["n_clusters"] == k, "kmeans"
            assert res.forced == dict(found=K0, target=k, method="kmeans", level=None, n_iter=km["n_iter"])
            assert np.array_equal(res.pi, base.pi) and np.array_equal(res.elbo, base.elbo)
        ref = AR.assign(E, info, list(tr), list(tl), constrained=True)
        Kref = ref["centroids"].shape[0]
        keep = ref["margin"] > 10 * bound
        left_out = int((~keep).sum())
        print(f"forced {clustering} k={k}: K0 {K0}, reachable {reachable}, speakers {res.n_speakers} (host {Kref}); {len(tr)} training rows; chunks left out "
              f"{left_out} of {len(st)}; forced {res.forced}")
        assert res.forced["found"] == K0 and res.forced["target"] == k and res.forced["method"] == method
        if reachable:
            assert res.n_speakers == k
        assert res.n_speakers == Kref and res.labels.max() < res.n_speakers <= k
        assert np.abs(np.linalg.norm(res.centroids.astype(np.float64), axis=1) - 1).max() <= 2.0 ** -22
        assert left_out <= 0.05 * len(st)
        labels, new, count, speakers, turns = DR.stitch(cls, st, ref["labels"], Kref, len(pcm))
        assert np.array_equal(labels[keep], res.labels[keep])
        if left_out == 0:
            assert np.array_equal(count, res.count) and np.array_equal(speakers, res.speakers) and turns == res.turns
            assert np.abs(ref["centroids"][np.argsort(new)] - res.centroids).max() <= 2.0 ** -23


# ------------------------------------------------------------------------------------------------ run_many
@pytest.mark.parametrize("clustering", ["ahc", "vbx"])
def test_run_many_equals_a_loop_of_run(diarizer, rec42, clustering):
    a, b = rec42, recording(30.0)
    recs, lps = [a[0], b[0], np.zeros(0, np.int16)], [a[1], b[1], np.zeros((0, F, 7), np.float32)]
    kw = dict(threshold=THRESHOLD[clustering], min_cluster_size=MIN_CLUSTER, clustering=clustering, constrained=True)
    plain = diarizer.run_many(recs, logp=lps, **kw)
    sync_plain = [dict(s) for s in diarizer.last_sync]
    many = diarizer.run_many(recs, logp=lps, speakers=2, **kw)
    sync = [dict(s) for s in diarizer.last_sync]
    print(f"run_many {clustering}: waits per pack {sync} (without speakers {sync_plain}); speakers {[r.n_speakers for r in many]} "
          f"(unbounded {[r.n_speakers for r in plain]}); forced {[r.forced for r in many]}")
    if clustering == "ahc":
        assert sync == sync_plain                                         # the level search is host integers on the Z already downloaded
    assert many[2].turns == [] and many[2].n_speakers == 0 and many[2].forced is None
    for r, (x, lp) in enumerate(zip(recs[:2], lps[:2])):
        one = diarizer.run(x, logp=lp, speakers=2, **kw)
        assert same_result(one, many[r], scores=False) and one.forced == many[r].forced
        assert np.abs(one.scores - many[r].scores).max() <= 2.0 ** -23
        if plain[r].n_speakers != 2:
            assert many[r].forced is not None and many[r].forced["target"] == 2 and many[r].forced["found"] == plain[r].n_speakers
        else:
            assert many[r].forced is None and same_result(plain[r], many[r])


# ------------------------------------------------------------------------------------------------ cluster_ranges, refusals
def test_cluster_ranges_takes_a_count(rec42, tmp_path, monkeypatch):
    monkeypatch.setenv("SPEAKERS_EMBEDDINGS_DIR", str(tmp_path / "store"))
    monkeypatch.setenv("SDK_CACHE_DIR", str(tmp_path / "cache"))
    monkeypatch.setenv("SDK_MODEL", "resnet34")
    be = importlib.import_module(f"{PKG}.backend").Backend()
    ranges = [(a, b) for _, a, b in LAYOUT]
    for clustering in ("ahc", "vbx"):
        kw = dict(threshold=THRESHOLD[clustering], min_cluster_size=MIN_CLUSTER, clustering=clustering)
        free = be.cluster_ranges(rec42[0], ranges, **kw)
        labels, wins, rl = be.cluster_ranges(rec42[0], ranges, speakers=2, **kw)
        print(f"cluster_ranges {clustering}: {len(wins)} windows, unbounded {int(free[0].max()) + 1} labels, speakers=2 gives {sorted(set(labels.tolist()))}")
        assert wins == free[1] and sorted(set(labels.tolist())) == [0, 1] and set(rl.tolist()) <= {0, 1}
        K0 = int(free[0].max()) + 1
        inside = be.cluster_ranges(rec42[0], ranges, speakers=(1, K0), **kw)
        assert np.array_equal(inside[0], free[0]) and np.array_equal(inside[2], free[2])
        with pytest.raises(ValueError, match="speakers="):
            be.cluster_ranges(rec42[0], ranges, speakers=(3, 2), **kw)


def test_refusals_come_before_any_device_work(diarizer, rec42):
    for bad in (0, (3, 2), "2"):
        with pytest.raises(ValueError, match="speakers="):
            diarizer.run(rec42[0], logp=rec42[1], speakers=bad)
        with pytest.raises(ValueError, match="speakers="):
            diarizer.run_many([rec42[0]], logp=[rec42[1]], speakers=bad)
    with pytest.raises(ValueError, match="speakers="):
        cluster.vbx_cluster(diarizer.eng, torch.zeros((4, D), device="cuda"), None, speakers=0)
