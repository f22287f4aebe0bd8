"""GPU checks of VBx with its HMM (sdk_vbx_hmm, Engine.vbx_hmm, cluster.vbx_cluster(loop_prob=...), Backend.cluster_ranges(clustering="vbx"))
against the loop-form reference of tests/vbx_hmm_ref.py on generated mixtures whose rows are laid out in speaker runs, so the chain matters.

Tolerances, as tests/test_vbx_gpu.py takes them.  What a different summation order costs is measured inside each test, per quantity: the
larger of the float64 reference's distance to its long-double run and to its run with every sum over rows and over speakers in descending
order (the yardstick).  A quantity passes within 8 x its yardstick + 4 ulp of its largest magnitude.  n_iter, keep, K and the hard labels
must be equal, after the reference alone has shown that none of those decisions is near a tie (the fixture conditions; a fixture that
breaks one FAILS).  Each test prints its figures before it asserts; profiles/r18_vbx_hmm_parity.txt records them as measured on an MI355X
(the worst ratio of any quantity and shape: 4.38, pi at n = 70, S = 300, loop_prob = 0).  The device's exp and log put no quantity over the
margin, so the yardstick has its two terms; vbx_hmm_ref.vbx_hmm(jitter=seed) is the third, should a later shape need it."""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vbx_hmm_ref as HR  # noqa: E402
import vbx_ref as VR  # noqa: E402

PKG = "speaker-diarization-toolkit_amd"
cluster = importlib.import_module(f"{PKG}.cluster")
P = importlib.import_module(f"{PKG}.plda")
LIB = importlib.import_module(f"{PKG}._lib")
pytestmark = pytest.mark.gpu
D0 = 128
MARGIN, ULPS = 8.0, 4.0
EPSILON = 1e-4
MAX_ITERS = 10                   # of the parity runs: the reference walks the chain row by row in Python
LONG_ITERS = 5                   # the same at n = 2049 (seconds per reference run; and there the ELBO still moves by more than 0.1 per iteration, far
                                 # from the stop threshold, where at 10 iterations its last step of 3e-7 lies inside 1e3 x the yardstick)

# (n, D, S, true speakers): the 64-row block edge (63, 65), the 64-lane stride crossed once (65) and twice (130), one row, one speaker, and
# S = 300 > 256, where the chain re-reads its rows instead of keeping the speakers in registers
CASES = [(1, 64, 1, 1), (2, 64, 2, 1), (63, 64, 7, 3), (65, 128, 65, 4), (300, 64, 130, 5), (2049, 128, 7, 3), (70, 64, 300, 4)]
LOOP = [0.0, 0.5, 0.99]
SEED = {}                        # (case, loop_prob) -> another seed, where the first broke a fixture condition
_mix, _cache = {}, {}


def iters(case):
    return LONG_ITERS if case[0] > 1000 else MAX_ITERS


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def mixture(case, seed=None):
    """The model and the mixture of one case, its rows in speaker runs: E [R, d_in], rows [n] ascending, init, true in TIME order."""
    key = (case, seed)
    if key not in _mix:
        n, D, S, n_true = case
        d_in = 192 if D == 64 else 256
        m = P.synthetic_plda(d_in, D0, seed=D + d_in, lda_dim=D)
        Phi_full, T_full = P.prepare(m.tr, m.psi, D0)
        sd = 100 + n + S if seed is None else seed
        E, rows, init, true = VR.mixture(sd, n, d_in, D0, D, S, n_true, (m.mean1, m.lda, m.mean2, m.mu, Phi_full), T_full)
        order = HR.speaker_runs(true, np.random.default_rng(sd + 1))
        E = E.copy()
        E[rows] = E[rows[order]]
        _mix[key] = (m, E, rows, init[order], true[order])
    return _mix[key]


def reference_runs(m, E, rows, init, S, loop_prob, **kw):
    runs = {}
    for name, dt, rev in (("f64", np.float64, False), ("ld", np.longdouble, False), ("rev", np.float64, True)):
        X = VR.transform(E[rows], m.mean1, m.lda, m.mean2, m.mu, m.T, dt)
        r = HR.vbx_hmm(X, m.Phi, init, S, loop_prob, dtype=dt, reverse=rev, **kw)
        c = VR.result(r["gamma"], r["pi"], E[rows], dt, rev)
        runs[name] = dict(gamma=r["gamma"], pi=r["pi"], elbo=r["elbo"], n_iter=r["n_iter"], cent64=c["cent"], keep=c["keep"], labels=c["labels"])
    return runs


def reference(case, loop_prob):
    """The reference runs of one case and loop probability (computed once, shared, never changed)."""
    key = (case, loop_prob)
    if key not in _cache:
        m, E, rows, init, true = mixture(case, SEED.get(key))
        _cache[key] = (m, E, rows, init, true, reference_runs(m, E, rows, init, case[2], loop_prob, epsilon=EPSILON, max_iters=iters(case)))
    return _cache[key]


def yardstick(runs, q):
    a = runs["f64"][q].astype(np.longdouble)
    out = 0.0
    for other in runs:
        if other != "f64":
            b = runs[other][q].astype(np.longdouble)
            out = max(out, float(np.abs(a - b).max()) if a.shape == b.shape and a.size else np.inf if a.shape != b.shape else 0.0)
    return out


def fixture_conditions(runs):
    """On the reference alone: the decisions that the exact checks compare are far from a tie."""
    ref = runs["f64"]
    y = yardstick(runs, "elbo")
    de = np.diff(ref["elbo"])
    near_stop = float(np.abs(de - EPSILON).min()) if len(de) else np.inf
    pi = ref["pi"]
    near_pi = int(((pi >= 1e-8) & (pi <= 1e-6)).sum())
    g = np.sort(ref["gamma"][:, ref["keep"]], axis=1)
    gap = float((g[:, -1] - g[:, -2]).min()) if g.shape[1] > 1 else np.inf
    print(f"  fixture: least |dELBO - epsilon| {near_stop:.3e} (must exceed 1e3 x the ELBO yardstick {y:.3e}); pi within a factor 10 of 1e-7: {near_pi}; "
          f"least gap of a row's two largest gammas {gap:.3e}; n_iter {[runs[k]['n_iter'] for k in runs]}; K {len(ref['keep'])}")
    assert np.isfinite(y) and near_stop > 1e3 * y, "bad fixture: an ELBO step lies at the stop threshold"
    assert near_pi == 0, "bad fixture: a speaker weight lies at the keep threshold"
    assert gap >= 1e-6, "bad fixture: a row's two largest responsibilities are tied"
    assert all(runs[k]["n_iter"] == ref["n_iter"] and np.array_equal(runs[k]["keep"], ref["keep"]) for k in runs)


def run_device(engine, m, E, rows, init, S, loop_prob, **kw):
    Ed, rd = dev(E), dev(rows)
    X = engine.plda_transform(Ed, rd, m)
    gamma, pi, elbo, n_iter, status = engine.vbx_hmm(X, m.device_arrays(Ed.device)["Phi"], dev(init), S, loop_prob, **kw)
    K, keep, labels, cent, cent64 = engine.vbx_centroids(gamma, pi, Ed, rd)
    torch.cuda.synchronize()
    n_it, Kn = int(n_iter.item()), int(K.item())
    return dict(gamma=gamma.cpu().numpy(), pi=pi.cpu().numpy(), elbo=elbo.cpu().numpy()[:n_it], elbo_all=elbo.cpu().numpy(), n_iter=n_it,
                status=int(status.item()), K=Kn, keep=keep.cpu().numpy(), labels=labels.cpu().numpy(), cent=cent.cpu().numpy(), cent64=cent64.cpu().numpy())


def compare(got, runs, quantities=("gamma", "pi", "elbo", "cent64")):
    ref = runs["f64"]
    K = len(ref["keep"])
    print(f"  gpu: status {got['status']} n_iter {got['n_iter']} (reference {ref['n_iter']}) K {got['K']} (reference {K})")
    assert got["status"] == 0 and got["n_iter"] == ref["n_iter"] and got["K"] == K
    assert np.array_equal(got["keep"][:K], ref["keep"]) and (got["keep"][K:] == -1).all()
    assert np.array_equal(got["labels"], ref["labels"])
    worst = {}
    for q in quantities:
        want = ref[q]
        have = got[q][:K] if q == "cent64" else got[q]
        y = yardstick(runs, q)
        tol = MARGIN * y + ULPS * float(np.spacing(np.abs(want).max()))
        err = float(np.abs(have - want).max())
        worst[q] = err / y if y > 0 else (0.0 if err == 0 else np.inf)
        print(f"  {q:7s} max|d| {err:.3e}  yardstick {y:.3e}  ratio {worst[q]:.2f}  tolerance {tol:.3e}")
        assert have.shape == want.shape and np.isfinite(have).all() and err <= tol, q
    print("  worst ratio per quantity: " + " ".join(f"{q}={v:.2f}" for q, v in worst.items()))


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("loop_prob", LOOP, ids=lambda p: f"P{p}")
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d-D%d-S%d" % c[:3])
def test_kernels_against_the_float64_reference(engine, case, loop_prob):
    n, D, S, n_true = case
    m, E, rows, init, true, runs = reference(case, loop_prob)
    print(f"vbx_hmm parity n={n} D={D} S={S} true={n_true} loop_prob={loop_prob}:")
    fixture_conditions(runs)
    got = run_device(engine, m, E, rows, init, S, loop_prob, epsilon=EPSILON, max_iters=iters(case))
    compare(got, runs)
    K = len(runs["f64"]["keep"])
    assert np.array_equal(got["cent"][:K], got["cent64"][:K].astype(np.float32)) and not got["cent"][K:].any() and not got["cent64"][K:].any()


# ------------------------------------------------------------------------------------------------ behaviour
BEHAVIOUR = (63, 64, 7, 3)


def test_two_runs_are_bit_identical(engine):
    for case in (BEHAVIOUR, (300, 64, 130, 5), (70, 64, 300, 4)):
        m, E, rows, init, _ = mixture(case)
        a = run_device(engine, m, E, rows, init, case[2], 0.99)
        b = run_device(engine, m, E, rows, init, case[2], 0.99)
        for q in ("gamma", "pi", "elbo_all", "cent", "cent64", "keep", "labels"):
            assert np.array_equal(a[q], b[q]), q
        assert a["n_iter"] == b["n_iter"] and a["K"] == b["K"]


def test_the_stop_test_runs_on_the_device(engine):
    m, E, rows, init, _, runs = reference(BEHAVIOUR, 0.99)
    S = BEHAVIOUR[2]
    free = run_device(engine, m, E, rows, init, S, 0.99, epsilon=-np.inf, max_iters=9)
    assert free["n_iter"] == 9 and free["status"] == 0                    # never stops early
    huge = run_device(engine, m, E, rows, init, S, 0.99, epsilon=np.inf)
    assert huge["n_iter"] == 2                                            # the test needs a previous ELBO: ii > 0
    assert np.array_equal(huge["elbo_all"][:2], free["elbo_all"][:2]) and not huge["elbo_all"][2:].any()
    # the launches after the stop leave the outputs untouched: the same as a call that ends there
    got = run_device(engine, m, E, rows, init, S, 0.99, epsilon=EPSILON)
    assert 2 < got["n_iter"] < 20 and got["n_iter"] == runs["f64"]["n_iter"]
    cut = run_device(engine, m, E, rows, init, S, 0.99, epsilon=EPSILON, max_iters=got["n_iter"])
    for q in ("gamma", "pi", "elbo", "cent64", "keep", "labels"):
        assert np.array_equal(got[q], cut[q]), q
    assert cut["n_iter"] == got["n_iter"] and not got["elbo_all"][got["n_iter"]:].any()


DYING = dict(seed=12, iters=80)


def test_a_speaker_that_dies_keeps_gamma_zero(engine):
    """The over-split speakers' weights fall every iteration and underflow to exactly 0 in the reference; from then on ln pi = -inf and the
    column of gamma is exactly 0, on the device as in the reference."""
    S = 7
    m = P.synthetic_plda(192, D0, seed=11, lda_dim=64)
    Phi_full, T_full = P.prepare(m.tr, m.psi, D0)
    E, rows, init, true = VR.mixture(DYING["seed"], 63, 192, D0, 64, S, 3, (m.mean1, m.lda, m.mean2, m.mu, Phi_full), T_full)
    order = HR.speaker_runs(true, np.random.default_rng(1))
    E[rows], init = E[rows[order]], init[order]
    ref = HR.vbx_hmm(VR.transform(E[rows], m.mean1, m.lda, m.mean2, m.mu, m.T), m.Phi, init, S, 0.9, max_iters=DYING["iters"], epsilon=-np.inf)
    assert (ref["pi"] == 0.0).sum() >= 1
    got = run_device(engine, m, E, rows, init, S, 0.9, epsilon=-np.inf, max_iters=DYING["iters"])
    dead = np.flatnonzero(got["pi"] == 0.0)
    print(f"dying speakers: pi = {got['pi'].tolist()}, K = {got['K']}")
    assert got["n_iter"] == DYING["iters"] and got["status"] == 0 and np.array_equal(dead, np.flatnonzero(ref["pi"] == 0.0))
    assert not got["gamma"][:, dead].any() and np.isfinite(got["gamma"]).all() and np.isfinite(got["elbo"]).all()
    assert got["K"] == S - len(dead) and not set(dead.tolist()) & set(got["keep"][:got["K"]].tolist())


def test_a_nan_row_sets_the_status_and_the_next_call_is_fine(engine):
    m, E, rows, init, _, runs = reference(BEHAVIOUR, 0.99)
    S = BEHAVIOUR[2]
    bad = E.copy()
    bad[rows[5], 17] = np.nan
    got = run_device(engine, m, bad, rows, init, S, 0.99)
    assert got["status"] & 1 and got["n_iter"] == 0 and not got["elbo_all"].any()
    with pytest.raises(ValueError, match="non-finite"):
        cluster.vbx_cluster(engine, dev(bad), m, rows=rows, loop_prob=0.99)
    ok = run_device(engine, m, E, rows, init, S, 0.99, epsilon=EPSILON, max_iters=MAX_ITERS)
    assert ok["status"] == 0 and ok["n_iter"] == runs["f64"]["n_iter"] and np.isfinite(ok["gamma"]).all()


def test_refusals_are_python_exceptions(engine):
    m, E, rows, init, _ = mixture(BEHAVIOUR)
    S = BEHAVIOUR[2]
    Ed, rd = dev(E), dev(rows)
    X = engine.plda_transform(Ed, rd, m)
    Phi = m.device_arrays(Ed.device)["Phi"]
    lab = dev(init)
    for bad in (float("nan"), -0.01, 1.0, 2.0):
        with pytest.raises(ValueError, match="loop_prob"):
            engine.vbx_hmm(X, Phi, lab, S, bad)
        with pytest.raises(ValueError, match="loop_prob"):
            cluster.vbx_cluster(engine, Ed, m, rows=rows, loop_prob=bad)
    with pytest.raises(ValueError, match="D=96 not supported"):
        engine.vbx_hmm(torch.zeros((63, 96), dtype=torch.float64, device="cuda"), Phi, lab, S, 0.5)
    with pytest.raises(ValueError, match="S=0"):
        engine.vbx_hmm(X, Phi, lab, 0, 0.5)
    with pytest.raises(ValueError, match="float64"):
        engine.vbx_hmm(X.float(), Phi, lab, S, 0.5)
    with pytest.raises(ValueError, match="int32"):
        engine.vbx_hmm(X, Phi, lab.long(), S, 0.5)
    with pytest.raises(ValueError, match="max_iters=0"):
        engine.vbx_hmm(X, Phi, lab, S, 0.5, max_iters=0)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.full((63, S), 7.0, dtype=torch.float64, device="cuda")
    out = torch.empty((20,), dtype=torch.float64, device="cuda")
    ws = torch.empty(256, dtype=torch.uint8, device="cuda")
    for lp, msg in ((float("nan"), "loop_prob"), (1.0, "loop_prob"), (0.5, "workspace of 256 bytes")):
        with pytest.raises(LIB.SdkError, match=msg):
            LIB.check(engine.lib.sdk_vbx_hmm(engine.ctx, X.data_ptr(), Phi.data_ptr(), lab.data_ptr(), 63, 64, S, 0.07, 0.8, 20, 1e-4, 7.0, lp, g.data_ptr(),
                                             out.data_ptr(), out.data_ptr(), lab.data_ptr(), lab.data_ptr(), ws.data_ptr(), 256, st), "sdk_vbx_hmm")
    torch.cuda.synchronize()
    assert bool((g == 7.0).all())                                         # nothing was launched


def test_vbx_cluster_loop_prob_zero_is_the_call_without_it(engine):
    m, E, rows, _, _ = mixture((300, 64, 130, 5))
    Ed = dev(E)
    a = cluster.vbx_cluster(engine, Ed, m, rows=rows)
    b = cluster.vbx_cluster(engine, Ed, m, rows=rows, loop_prob=0.0)
    assert a.n_iter == b.n_iter and a.n_speakers == b.n_speakers
    for f in ("labels", "pi", "elbo", "keep", "init_labels"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    for f in ("cent", "cent64", "gamma"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f


def test_vbx_cluster_with_the_chain_from_the_linkage(engine):
    """cluster.vbx_cluster(loop_prob=0.99) end to end: the device's own linkage cut, then the reference chained from that cut."""
    case = (300, 128, 65, 4)
    m, E, rows, _, true = mixture(case)
    res = cluster.vbx_cluster(engine, dev(E), m, rows=rows, loop_prob=cluster.VBX_LOOP_PROB)
    init = res.init_labels
    S = int(init.max()) + 1
    runs = reference_runs(m, E, rows, init, S, cluster.VBX_LOOP_PROB)
    print(f"vbx_cluster(loop_prob=0.99): S={S} n_iter={res.n_iter} K={res.n_speakers} keep={res.keep.tolist()}")
    fixture_conditions(runs)
    K = res.n_speakers
    cent64 = np.zeros((S, E.shape[1]))
    cent64[:K] = res.cent64.cpu().numpy()
    got = dict(status=0, n_iter=res.n_iter, K=K, keep=np.concatenate([res.keep, np.full(S - K, -1, np.int32)]), labels=res.labels,
               gamma=res.gamma.cpu().numpy(), pi=res.pi, elbo=res.elbo, cent64=cent64)
    compare(got, runs)
    assert S > 1 and res.gamma.shape == (300, S) and res.cent.shape == (K, E.shape[1])
    for k in range(K):                                                    # a speaker is one true speaker, but for single rows that the chain keeps with their neighbours
        assert np.sort(np.bincount(true[res.labels == k]))[:-1].sum() <= 0.02 * (res.labels == k).sum()


# ------------------------------------------------------------------------------------------------ Backend.cluster_ranges(clustering="vbx")
RATE = 16000
VOICES = [(101, 100.0, 700.0, 4.0), (202, 2500.0, 4000.0, 9.0), (303, 5000.0, 7500.0, 2.0)]


def voice(seed: int, lo: float, hi: float, am: float, n: int) -> np.ndarray:
    """A stand-in voice: seeded noise limited to the band lo .. hi Hz, gated on and off am times a second."""
    rng = np.random.default_rng(seed)
    X = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1 / RATE)
    X[(f < lo) | (f > hi)] = 0
    t = np.arange(n) / RATE
    x = np.fft.irfft(X, n) * (0.05 + 0.5 * (1 + np.tanh(4 * np.sin(2 * np.pi * am * t))))
    return x / np.abs(x).max() * 0.3


def test_cluster_ranges_with_vbx(tmp_path, monkeypatch):
    from scipy.cluster.hierarchy import linkage
    monkeypatch.setenv("SPEAKERS_EMBEDDINGS_DIR", str(tmp_path / "store"))
    monkeypatch.setenv("SDK_CACHE_DIR", str(tmp_path / "cache"))
    monkeypatch.setenv("SDK_MODEL", "resnet34")
    be = importlib.import_module(f"{PKG}.backend").Backend()
    turns = [0, 1, 2, 0, 1, 2]                                            # three voices alternating, 3 s each
    x = np.random.default_rng(7).normal(0, 0.001, 3 * RATE * len(turns))
    for i, v in enumerate(turns):
        x[3 * RATE * i:3 * RATE * (i + 1)] += voice(VOICES[v][0] + i, *VOICES[v][1:], 3 * RATE)
    samples = np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)
    ranges = [(3.0 * i, 3.0 * (i + 1)) for i in range(len(turns))] + [(18.0, 18.2)]
    E, _, _, wins, _ = be.embed_ranges(samples, ranges)
    Eh = E.cpu().numpy()
    W = len(wins)
    assert W >= len(turns) and [w[1] for w in wins] == sorted(w[1] for w in wins)      # the windows are in time order
    Z = linkage(Eh.astype(np.float64), "centroid")
    h = Z[:, 2]
    best = max(range(3, 7), key=lambda S: h[len(h) - S + 1] - h[len(h) - S])           # 3 .. 6 initial clusters: the widest gap between merge heights
    threshold = 0.5 * (h[len(h) - best] + h[len(h) - best + 1])
    plda = be.diarizer().plda_model()
    assert plda.d_in == Eh.shape[1]
    init = cluster.fcluster_distance(Z, threshold)
    S = int(init.max()) + 1
    runs = reference_runs(plda, Eh, np.arange(W), init, S, cluster.VBX_LOOP_PROB)
    print(f"cluster_ranges(vbx): {W} windows, S={S} (threshold {threshold:.4f}, cut gap {np.abs(h - threshold).min():.3e})")
    fixture_conditions(runs)
    labels, wins2, rl = be.cluster_ranges(samples, ranges, threshold=threshold, clustering="vbx")
    assert wins2 == wins and labels.shape == (W,) and labels.dtype == np.int32 and rl.shape == (len(ranges),) and rl.dtype == np.int32 and rl[-1] == -1
    assert np.array_equal(labels, runs["f64"]["labels"])
    for ri in range(len(turns)):
        lab = [int(v) for (r, _, _), v in zip(wins, labels) if r == ri]
        assert rl[ri] == int(np.argmax(np.bincount(lab)))
    same = be.cluster_ranges(samples, ranges, threshold=threshold, clustering="vbx", loop_prob=cluster.VBX_LOOP_PROB, plda=plda)
    assert np.array_equal(same[0], labels) and np.array_equal(same[2], rl)
    # "ahc" is the call without the argument
    a, b = be.cluster_ranges(samples, ranges, threshold=0.3, min_cluster_size=2), be.cluster_ranges(samples, ranges, threshold=0.3, min_cluster_size=2,
                                                                                                  clustering="ahc")
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
    with pytest.raises(ValueError, match="clustering='spectral'"):
        be.cluster_ranges(samples, ranges, clustering="spectral")
