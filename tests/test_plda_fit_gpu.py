"""GPU checks of the PLDA training's device half (sdk_plda_fit_stats, sdk_plda_project; plda.fit) against the loop-form reference of
tests/plda_fit_ref.py on rows from a planted two-covariance model.

Tolerances: the convention of tests/test_vbx_gpu.py.  Per quantity the yardstick is the larger distance of the float64 reference to its
long-double run and to its run with every sum over rows in descending order; a quantity passes within 8 x yardstick + 4 ulp of its largest
magnitude.  Model-level quantities (Phi, objf, W, B) take the same yardstick after the yardstick runs' statistics have gone through the same
host solve (plda.fit_from_stats).  Counts are exact, the scatter exactly symmetric, a second call bit-identical.  Each test prints its figures
before it asserts; profiles/r28_plda_fit_parity.txt records them as measured on an MI355X."""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import partial_width as PW  # noqa: E402
import plda_fit_ref as FR  # noqa: E402

PKG = "speaker-diarization-toolkit_amd"
P = importlib.import_module(f"{PKG}.plda")
cluster = importlib.import_module(f"{PKG}.cluster")
pytestmark = pytest.mark.gpu
MARGIN, ULPS = 8.0, 4.0
QUANT = ("sums", "total", "scatter")

# (N, d, K): one row block and several (RB = 512), d below, at and above the 64-wide macro tile, classes of one row, unused ids; the last two: the
# widths at which a thread's second column (tid + 256) is live for wave 0 only (320) and for every wave but the last (448).  Checked on the CPU
# (tests/test_plda_fit_cpu.py prints it): without the columns 256.. of the rows the reference's sums, total and scatter move by more than
# 1e13 x their tolerances
STATS_CASES = [(2, 64, 1), (63, 64, 7), (65, 192, 65), (300, 100, 12), (2049, 256, 40), (2049, 512, 2), (65, 320, 9), (300, 448, 12)]
_cache = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rows_of(case):
    N, d, K = case
    d_gen = d if d % 64 == 0 else 128
    if case == (65, 192, 65):
        E, lab, _ = FR.labelled_rows(7, N, d_gen, K, singles=range(K))
    elif case == (2049, 256, 40):
        E, lab, _ = FR.labelled_rows(8, N, d_gen, K, unused=(3, 39), singles=(5,), scramble=True)
    else:
        E, lab, _ = FR.labelled_rows(N + d, N, d_gen, K)
    return E, lab


def reference(case):
    """The rows and the reference runs of one case (computed once, shared, never changed): the fp32 source with the stage-1 transform fused
    (d a multiple of 64), and the float64 source (the same rows, already transformed; at d = 100 their first 100 columns)."""
    if case not in _cache:
        N, d, K = case
        E, lab = rows_of(case)
        mean1 = E.astype(np.float64).mean(0)
        X64 = np.ascontiguousarray(FR.stage1_rows(E, mean1)[:, :d])
        runs64 = {"f64": FR.stats(X64, lab, K), "ld": FR.stats(X64, lab, K, np.longdouble), "rev": FR.stats(X64, lab, K, reverse=True)}
        runs32 = None
        if d % 64 == 0:
            runs32 = {"f64": runs64["f64"], "rev": runs64["rev"], "ld": FR.stats(FR.stage1_rows(E, mean1, np.longdouble), lab, K, np.longdouble)}
        _cache[case] = (E, lab, mean1, X64, runs32, runs64)
    return _cache[case]


def yardstick(runs, q):
    a = np.asarray(runs["f64"][q]).astype(np.longdouble)
    return max(float(np.abs(a - np.asarray(runs[o][q]).astype(np.longdouble)).max()) for o in ("ld", "rev"))


def tolerance(runs, q):
    return MARGIN * yardstick(runs, q) + ULPS * float(np.spacing(np.abs(np.asarray(runs["f64"][q], dtype=np.float64)).max()))


def stats_weight(case) -> float:
    """partial_width.weight of a statistics case wider than 256 columns, on the reference alone: the float64 rows without their columns 256..."""
    N, d, K = case
    _, lab, _, X64, _, runs64 = reference(case)
    return FR.second_column_weight("plda fit statistics N=%d d=%d K=%d" % case, runs64["f64"], FR.stats(PW.first_columns(X64), lab, K),
                                   {q: tolerance(runs64, q) for q in QUANT})


def within(name, have, runs, q):
    want = np.asarray(runs["f64"][q], dtype=np.float64)
    y = yardstick(runs, q)
    tol = tolerance(runs, q)
    err = float(np.abs(have - want).max())
    print(f"  {name:10s} max|d| {err:.3e}  yardstick {y:.3e}  ratio {err / y if y > 0 else 0.0 if err == 0 else np.inf:.2f}  tolerance {tol:.3e}")
    assert have.shape == want.shape and np.isfinite(have).all() and err <= tol, name


def host(s):
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in s.items()}


def check_stats(got, runs, K):
    assert int(got["status"][0]) == 0
    assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], runs["f64"]["counts"])
    for q in QUANT:
        within(q, got[q], runs, q)
    assert np.array_equal(got["scatter"], got["scatter"].T), "the scatter is not exactly symmetric"


# ------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("case", STATS_CASES, ids=lambda c: "N%d-d%d-K%d" % c)
def test_statistics_against_the_float64_reference(engine, case):
    N, d, K = case
    E, lab, mean1, X64, runs32, runs64 = reference(case)
    labd = dev(lab)
    print(f"plda fit statistics N={N} d={d} K={K}: counts min {runs64['f64']['counts'].min()} max {runs64['f64']['counts'].max()}")
    if case == (65, 192, 65):
        assert (runs64["f64"]["counts"] == 1).all()
    if case == (2049, 256, 40):
        assert runs64["f64"]["counts"][3] == 0 and runs64["f64"]["counts"][39] == 0 and (np.diff(lab) < 0).any()
    if d in PW.WIDTHS:
        stats_weight(case)
    sources = [("float64 rows", dev(X64), None, runs64)]
    if runs32 is not None:
        sources.append(("fp32 rows, transform fused", dev(E), dev(mean1), runs32))
    for name, rows, m1, runs in sources:
        print(f" {name}:")
        got = host(engine.plda_fit_stats(rows, labd, K, mean1=m1))
        check_stats(got, runs, K)
        again = host(engine.plda_fit_stats(rows, labd, K, mean1=m1))
        for q in ("counts",) + QUANT:
            assert np.array_equal(got[q], again[q]), f"{q}: a second call differs"
        # the same rows in another order: the same counts (and sums within the tolerance)
        perm = np.random.default_rng(N).permutation(N)
        other = host(engine.plda_fit_stats(rows[dev(perm)].contiguous(), dev(lab[perm]), K, mean1=m1))
        assert np.array_equal(other["counts"], got["counts"])
        check_stats(other, runs, K)
        # without the scatter, and without labels: the other outputs bit for bit
        bare = host(engine.plda_fit_stats(rows, labd, K, mean1=m1, scatter=False))
        assert bare["scatter"] is None and all(np.array_equal(bare[q], got[q]) for q in ("counts", "sums", "total"))
        tot = host(engine.plda_fit_stats(rows, mean1=m1, scatter=False))
        assert np.array_equal(tot["total"], got["total"])


def test_the_mean_pass_takes_the_rows_as_they_are(engine):
    case = (2049, 256, 40)
    E, lab, mean1, _, _, _ = reference(case)
    runs = {"f64": FR.stats(E, None, 0, scatter=False), "ld": FR.stats(E, None, 0, np.longdouble, scatter=False),
            "rev": FR.stats(E, None, 0, reverse=True, scatter=False)}
    got = host(engine.plda_fit_stats(dev(E), scatter=False))
    within("total", got["total"], runs, "total")


def test_a_label_outside_the_range_raises_and_the_next_call_is_fine(engine):
    case = (63, 64, 7)
    N, d, K = case
    E, lab, mean1, X64, runs32, _ = reference(case)
    for bad_value in (-1, K):
        bad = lab.copy()
        bad[11] = bad_value
        with pytest.raises(ValueError, match="labels must lie in"):
            engine.plda_fit_stats(dev(E), dev(bad), K, mean1=dev(mean1))
        # unchecked, the library itself never indexes with it: status bit 1, the row in no class
        got = host(engine.plda_fit_stats(dev(E), dev(bad), K, mean1=dev(mean1), check_labels=False))
        assert int(got["status"][0]) == 1 and int(got["counts"].sum()) == N - 1
        with pytest.raises(ValueError, match="labels must lie in"):
            P.fit(engine, dev(E), dev(bad), 64, 64, 2, K=K)
    check_stats(host(engine.plda_fit_stats(dev(E), dev(lab), K, mean1=dev(mean1))), runs32, K)


# ------------------------------------------------------------------------------------------------ projection
# the last two: d_in = 320 into D0 = 300 (a thread's second column partial over the input AND the output) and 448 into 448.  Checked on the CPU
# (tests/test_plda_fit_cpu.py prints it): without the input columns 256.. the reference's x2 moves by more than 1e13 x its tolerance
PROJECTION_CASES = [(1, 64, 64), (63, 192, 100), (2049, 256, 128), (5, 512, 300), (63, 320, 300), (5, 448, 448)]


def projection_reference(case):
    """-> (E, the synthetic model, x2 in float64, x2 in long double) of one projection case."""
    N, d_in, D0 = case
    E, _, _ = FR.labelled_rows(N + D0, N, d_in, 1)
    m = P.synthetic_plda(d_in, D0, seed=N, lda_dim=64)
    return E, m, FR.project(E, m.mean1, m.lda, m.mean2), FR.project(E, m.mean1, m.lda, m.mean2, np.longdouble)


def projection_weight(case, E, m, ref, ld) -> float:
    runs = {"f64": {"x2": ref}, "ld": {"x2": ld}, "rev": {"x2": ref}}
    return FR.second_column_weight("plda projection N=%d %d -> %d" % case, {"x2": ref}, {"x2": FR.project(PW.first_columns(E), m.mean1, m.lda, m.mean2)},
                                   {"x2": tolerance(runs, "x2")})


@pytest.mark.parametrize("case", PROJECTION_CASES, ids=lambda c: "N%d-%dto%d" % c)
def test_projection(engine, case):
    N, d_in, D0 = case
    E, m, ref, ld = projection_reference(case)
    if d_in in PW.WIDTHS:
        projection_weight(case, E, m, ref, ld)
    got = engine.plda_project(dev(E), dev(m.mean1), dev(m.lda), dev(m.mean2))
    torch.cuda.synchronize()
    print(f"plda projection N={N} {d_in} -> {D0}:")
    within("x2", got.cpu().numpy(), {"f64": {"x2": ref}, "ld": {"x2": ld}, "rev": {"x2": ref}}, "x2")
    # sdk_plda_transform's first two steps: with mu = 0 and T = I its output is x2[:, :D]
    D = 128 if D0 >= 128 else 64
    ident = P.Plda(m.mean1, m.lda, m.mean2, np.zeros(D0), np.eye(D0), np.ones(D0), D, Phi=np.ones(D), T=np.eye(D, D0))
    X = engine.plda_transform(dev(E), dev(np.arange(N, dtype=np.int32)), ident)
    torch.cuda.synchronize()
    assert torch.equal(X, got[:, :D].contiguous())


# ------------------------------------------------------------------------------------------------ the whole fit
FIT_CASES = [(600, 64, 64, 64, 80), (3000, 192, 100, 64, 150)]
VBX_FACTORS = {FIT_CASES[0]: dict(Fa=0.3, Fb=1.0), FIT_CASES[1]: {}}
_fits = {}


def fit_reference(case):
    if case not in _fits:
        N, d_in, D0, lda_dim, K = case
        E, lab, planted = FR.labelled_rows(1000 + N, N, d_in, K, unused=(2, K - 1), singles=(0, 7))
        total0 = E.astype(np.float64).sum(0)
        runs = {}
        for name, dt, rev in (("f64", np.float64, False), ("ld", np.longdouble, False), ("rev", np.float64, True)):
            model, f = P.fit_from_stats(
                FR.stats(E, None, 0, dt, rev, scatter=False)["total"] if name != "f64" else total0,
                lambda mean1: FR.stats(FR.stage1_rows(E, mean1, dt), lab, K, dt, rev),
                lambda mean1, lda, mean2: FR.stats(FR.project(E, mean1, lda, mean2, dt), lab, K, dt, rev), N, D0, lda_dim, 10)
            runs[name] = dict(Phi=model.Phi, objf=f.objf, W=f.W, B=f.B, eig=f.eigenvalues, psi=model.psi,
                              **{f"s1_{q}": f.stats1[q] for q in QUANT}, **{f"s2_{q}": f.stats2[q] for q in QUANT})
        _fits[case] = (E, lab, planted, runs)
    return _fits[case]


@pytest.mark.parametrize("case", FIT_CASES, ids=lambda c: "N%d-%dto%d-D%d-K%d" % c)
def test_fit_against_fit_host(engine, case):
    N, d_in, D0, lda_dim, K = case
    E, lab, planted, runs = fit_reference(case)
    ref = runs["f64"]
    print(f"plda fit N={N} d_in={d_in} D0={D0} lda_dim={lda_dim} K={K}:")
    # fixture conditions, on the reference alone
    if D0 < d_in:
        y = yardstick(runs, "eig")
        gap = float((ref["eig"][D0 - 1] - ref["eig"][D0]) / ref["eig"][D0 - 1])
        print(f"  fixture: relative gap of stage-1 eigenvalues {D0} and {D0 + 1}: {gap:.3e} (must exceed 1e3 x their yardstick {y:.3e})")
        assert gap > 1e3 * y, "bad fixture: the LDA subspace is not separated"
    print(f"  fixture: least psi {ref['psi'].min():.3e} (floor 1e-12)")
    assert ref["psi"].min() > 1e-12, "bad fixture: a psi lies at the floor"
    model_h, fh = P.fit_host(E, lab, D0, lda_dim, 10, K=K)
    model_d, fd = P.fit(engine, dev(E), dev(lab), D0, lda_dim, 10, K=K)
    assert np.array_equal(fd.counts, fh.counts) and fd.n_classes == fh.n_classes == K - 2 and fd.n_rows == N
    for st, a, b in (("s1", fd.stats1, fh.stats1), ("s2", fd.stats2, fh.stats2)):
        for q in QUANT:
            y = yardstick(runs, f"{st}_{q}")
            want = ref[f"{st}_{q}"]                                       # the loop reference, and fit_host's numpy statistics
            tol = MARGIN * y + ULPS * float(np.spacing(np.abs(want).max()))
            err, err_h, host_err = (float(np.abs(u - v).max()) for u, v in ((a[q], want), (a[q], b[q]), (b[q], want)))
            print(f"  {st} {q:8s} fit - reference {err:.3e}  fit - fit_host {err_h:.3e}  fit_host - reference {host_err:.3e}  yardstick {y:.3e}  tolerance {tol:.3e}")
            assert err <= tol and err_h <= tol and host_err <= tol, (st, q)
    for q, a, b in (("Phi", model_d.Phi, model_h.Phi), ("objf", fd.objf, fh.objf), ("W", fd.W, fh.W), ("B", fd.B, fh.B)):
        y = yardstick(runs, q)
        tol = MARGIN * y + ULPS * float(np.spacing(np.abs(b).max()))
        err = float(np.abs(a - b).max())
        print(f"  {q:11s} max|d| {err:.3e}  yardstick {y:.3e}  tolerance {tol:.3e}")
        assert a.shape == b.shape and np.isfinite(a).all() and err <= tol, q
    # a fresh mixture from the same planted model clusters the same with either model.  The rows are noisy enough that the initial cut
    # leaves every row alone (160 clusters); VBX_FACTORS are chosen on the CPU reference (tests/vbx_ref.py on fit_host's model) so that the
    # four true speakers survive: at d_in = 64 the default Fa = 0.07 merges them all into one, which would say nothing
    rng = np.random.default_rng(5)
    truth = np.repeat(np.arange(4), 40)
    Em = dev(planted.rows(rng, planted.speakers(rng, 4), truth))
    kw = VBX_FACTORS[case]
    rh = cluster.vbx_cluster(engine, Em, model_h, **kw)
    assert rh.n_speakers > 1 and int(rh.init_labels.max()) > 0, "bad fixture: the mixture is one cluster, the labels say nothing"
    g = np.sort(rh.gamma.cpu().numpy()[:, rh.keep], axis=1)
    gap = float((g[:, -1] - g[:, -2]).min())
    purity = sum(int(np.bincount(truth[rh.labels == k]).max()) for k in range(rh.n_speakers)) / len(truth)
    print(f"  vbx on a fresh mixture ({kw or 'default factors'}, {int(rh.init_labels.max()) + 1} initial clusters): {rh.n_speakers} speakers, purity {purity:.3f}, "
          f"least gap of a row's two largest gammas {gap:.3e}")
    assert gap >= 1e-6, "bad fixture: a row's two largest responsibilities are tied"
    rd = cluster.vbx_cluster(engine, Em, model_d, **kw)
    assert rd.n_speakers == rh.n_speakers and np.array_equal(rd.labels, rh.labels)


# ------------------------------------------------------------------------------------------------ from recordings to the two files
import test_diarize_gpu as TG  # noqa: E402

dzm = importlib.import_module(f"{PKG}.diarize")
DH = importlib.import_module(f"{PKG}.diarize_host")
SC = importlib.import_module(f"{PKG}.score")
seg = importlib.import_module(f"{PKG}.segmentation")
RATE, STEP_S = 16000, 1.0
_recs = {}


def recording(i, n_s=20):
    """A generated two-speaker recording with an overlap, its injected logp and its exact reference: speaker a from 0.5 s, b to the end."""
    if i not in _recs:
        rng = np.random.default_rng(900 + i)
        n = n_s * RATE
        cut = float(rng.uniform(5.0, 8.0))
        layout = [(0, 0.5, cut + 1.0), (1, cut, n_s - 0.5)]
        x = rng.normal(0, 0.001, n)
        for v, a, b in layout:
            i0, i1 = int(a * RATE), int(b * RATE)
            lo = float(rng.uniform(100.0, 5000.0))
            x[i0:i1] += TG.voice(int(rng.integers(1 << 30)), lo, lo + float(rng.uniform(500.0, 2500.0)), float(rng.uniform(2.0, 9.0)), i1 - i0)
        pcm = np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)
        st = seg.chunk_starts(n, STEP_S)
        cls = FR.class_table(layout, st)
        _recs[i] = (pcm, st, cls, TG.logp_of(cls), [(a, b, "ab"[v]) for v, a, b in layout])
    return _recs[i]


def restated_labels(pcm, st, cls, turns, T4):
    """Every row's reference speaker by tests/plda_fit_ref.py's loops (the training mask and the rasterised reference are the package's)."""
    _, info = DH.masks_host(cls, T4)
    G = DH.global_frames(len(pcm))
    merged, names = SC.prepare_reference(turns)
    mask, _ = SC.reference_masks_host(merged, G)
    dense = np.array([[(int(m) >> r) & 1 for m in mask] for r in range(len(names))], bool).reshape(len(names), G)
    return FR.label_rows(cls, st, DH.training_mask(info, cls.shape[1]), dense), names


def test_plda_rows_labels_equal_the_restatement(engine):
    rn = importlib.import_module(f"{PKG}.resnet")
    net = rn.ResNet34(engine, rn.synthetic_weights(0), precision=0)
    d = dzm.Diarizer(engine, None, net)
    recs = [recording(i) for i in range(4)]
    got = d.plda_rows([r[0] for r in recs], [r[4] for r in recs], step_s=STEP_S, logp=[r[3] for r in recs])
    T4 = net.last_map_frames(TG.T_CHUNK)
    n_all = 0
    for i, (pcm, st, cls, _, turns) in enumerate(recs):
        want, names = restated_labels(pcm, st, cls, turns, T4)
        rows = np.flatnonzero(want >= 0)
        mine = got["recording"] == i
        assert got["names"][i] == names == ["a", "b"]
        assert np.array_equal(got["row"][mine], rows) and np.array_equal(got["speaker"][mine], want[rows])
        assert set(want[rows].tolist()) == {0, 1}                                    # both speakers have rows
        n_all += len(rows)
    E = got["E"]
    print(f"plda_rows: {n_all} labelled rows of {got['n_training']} training rows, {got['n_dropped']} dropped")
    assert E.is_cuda and E.dtype == torch.float32 and tuple(E.shape) == (n_all, net.cfg.embed_dim) and got["n_dropped"] == got["n_training"] - n_all
    assert torch.allclose(E.norm(dim=1), torch.ones(n_all, device=E.device), atol=1e-5)
    # the rows are those of the pipeline's own embedding pass
    one = d.plda_rows([recs[2][0]], [recs[2][4]], step_s=STEP_S, logp=[recs[2][3]])
    assert torch.equal(one["E"], E[torch.from_numpy(np.flatnonzero(got["recording"] == 2)).to(E.device)])


def test_train_plda_writes_a_model_that_vbx_runs_on(engine, monkeypatch, tmp_path):
    """Four two-speaker recordings are 8 classes, fewer than the D0 + 1 >= 65 the rule asks for: refused.  48 such recordings (96 classes)
    train; the two files come back bit for bit, and a Backend pointed at them diarizes with clustering="vbx"."""
    for k in ("SDK_MODEL", "SDK_NO_TORCH", "SDK_PRECISION", "SDK_RESNET_WEIGHTS", "SDK_SEGMENTATION_WEIGHTS", "SDK_DIARIZE_MODEL", "SDK_PLDA",
              "SDK_PLDA_TRANSFORM", "SDK_PLDA_DIM"):
        monkeypatch.delenv(k, raising=False)
    be = importlib.import_module(f"{PKG}.backend").Backend()
    recs = [recording(i) for i in range(48)]
    args = lambda n: ([r[0] for r in recs[:n]], [r[4] for r in recs[:n]])  # noqa: E731
    with pytest.raises(ValueError, match="classes with a row"):
        be.train_plda(*args(4), logp=[r[3] for r in recs[:4]], D0=64, lda_dim=64, step_s=STEP_S)
    uris = [f"rec{i:02d}" for i in range(48)]
    out = tmp_path / "model"
    model, report = be.train_plda(*args(48), uris=uris, out_dir=out, D0=64, lda_dim=64, n_iters=5, step_s=STEP_S, logp=[r[3] for r in recs])
    print(f"train_plda: {report['rows_used']} rows used, {report['rows_dropped']} dropped, {report['classes']} classes, objf {report['objf'].tolist()}")
    assert report["classes"] == 96 and report["class_keys"][:2] == [("rec00", "a"), ("rec00", "b")] and report["rows_used"] == int(report["counts"].sum())
    assert report["objf"].shape == (5,) and np.isfinite(report["objf"]).all() and report["objf"][-1] > report["objf"][0]
    assert report["transform_npz"] == out / "xvec_transform.npz" and report["plda_npz"] == out / "plda.npz"
    back = P.load_plda(report["transform_npz"], report["plda_npz"], 64)
    for k in ("mean1", "lda", "mean2", "mu", "tr", "psi", "Phi", "T"):
        assert np.array_equal(getattr(back, k), getattr(model, k)), k
    merged, report2 = be.train_plda(*args(48), uris=uris, D0=64, lda_dim=64, n_iters=2, step_s=STEP_S, logp=[r[3] for r in recs],
                                    speaker_key=lambda uri, name: (uri if int(uri[3:]) >= 2 else "rec00", name))
    assert report2["classes"] == 94 and report2["rows_used"] == report["rows_used"] and "plda_npz" not in report2
    monkeypatch.setenv("SDK_PLDA_TRANSFORM", str(report["transform_npz"]))
    monkeypatch.setenv("SDK_PLDA", str(report["plda_npz"]))
    monkeypatch.setenv("SDK_PLDA_DIM", "64")
    be2 = importlib.import_module(f"{PKG}.backend").Backend()
    assert np.array_equal(be2.diarizer().plda_model().tr, model.tr)
    res = be2.diarize(recs[0][0], step_s=STEP_S, logp=recs[0][3], clustering="vbx", threshold=0.6)
    print(f"vbx on the trained model: {res.n_speakers} speakers, elbo {None if res.elbo is None else res.elbo.tolist()}")
    assert res.n_speakers >= 1 and res.elbo is not None and np.isfinite(res.elbo).all() and len(res.turns) > 0
