"""CPU checks of the calibration part of trials.py (calib_sums_host, objective, newton_fit, fit_from_counts, pav_min_cllr, the driver
calibration_from_passes, save / load) against the independent long-double restatement of tests/calib_ref.py, and of the application of a
calibration in rules.py (SDK_SCORE_CALIBRATION: its refusals, and rows that gain exactly two keys - on the torch-free path too)."""
from __future__ import annotations

import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calib_ref as CR  # noqa: E402
from conftest import sub  # noqa: E402

T = sub("trials")
RULES = sub("rules")
U53 = 2.0 ** -53
PRIOR = T.effective_prior()


def two_gaussians(n=20000, seed=3, sep=2.0):
    rng = np.random.default_rng(seed)
    S = np.concatenate([rng.normal(+sep / 2, 1.0, n), rng.normal(-sep / 2, 1.0, n)])
    cls = np.concatenate([np.ones(n, np.int64), np.zeros(n, np.int64)])
    return S, cls


# ---- a pass ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,c", [(1.0, 0.0), (0.37, -2.5), (6.0, 40.0)])
def test_host_sums_agree_with_the_long_double_reference(a, c):
    rng = np.random.default_rng(5)
    S = rng.normal(0.0, 4.0, 3000)
    S[:8] = [(40 - c) / a, (-40 - c) / a, (750 - c) / a, (-750 - c) / a, np.nan, np.inf, -np.inf, 0.0]        # m = +-40, +-750 for both classes
    cls = rng.integers(-1, 2, 3000)
    cls[:8] = [1, 1, 0, 0, 1, 0, 1, 0]
    got, ref = T.calib_sums_host(S, cls, a, c), CR.sums(S, cls, a, c)
    assert got.n.tolist() == ref["n"] and got.nonfinite.tolist() == ref["nonfinite"] == [1, 2] and got.excluded == ref["excluded"] > 0
    # per term: exp and log1p within 1 ulp, the division, three multiplications and two additions correctly rounded (< 12 u in all); numpy's
    # pairwise sum adds at most log2(n) + 8 roundings to a term
    bound = (12 + math.log2(len(S)) + 8) * U53 * ref["mag"].astype(np.float64) * (1 + 1e-9)
    err = np.abs((got.sums.astype(np.longdouble) - ref["sums"]).astype(np.float64))
    assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()
    empty = T.calib_sums_host(S, np.where(cls == 1, -1, cls), a, c)                    # no target left
    assert empty.n[1] == 0 and not empty.sums[1].any() and empty.n[0] == got.n[0] and np.array_equal(empty.sums[0], got.sums[0])
    with pytest.raises(ValueError, match="both classes"):
        T.objective(empty, PRIOR)
    with pytest.raises(ValueError, match="both classes"):
        T.cllr_of(empty)


def test_gradient_and_hessian_are_those_of_J():
    S, cls = two_gaussians(2000, seed=8)
    theta = math.log(PRIOR / (1 - PRIOR))
    J = lambda a, b: float(CR.objective(CR.sums(S, cls, a, b + theta), PRIOR)[0])        # noqa: E731
    a, b, h = 0.8, 0.3, 1e-4
    _, g, H = T.objective(T.calib_sums_host(S, cls, a, b + theta), PRIOR)
    num_g = np.asarray([(J(a + h, b) - J(a - h, b)) / (2 * h), (J(a, b + h) - J(a, b - h)) / (2 * h)])
    assert np.allclose(g, num_g, rtol=1e-6, atol=1e-9)
    grad = lambda a, b: T.objective(T.calib_sums_host(S, cls, a, b + theta), PRIOR)[1]        # noqa: E731
    num_H = np.stack([(grad(a + h, b) - grad(a - h, b)) / (2 * h), (grad(a, b + h) - grad(a, b - h)) / (2 * h)])
    assert np.allclose(H, num_H, rtol=1e-6, atol=1e-9) and H[0, 1] == H[1, 0]
    rg, rH = CR.objective(CR.sums(S, cls, a, b + theta), PRIOR)[1:]
    assert np.allclose(g, rg.astype(np.float64), rtol=1e-12) and np.allclose(H, rH.astype(np.float64), rtol=1e-12)


# ---- the fit -----------------------------------------------------------------------------------------------------------------------------
def host_calibration(S, cls, lo, hi, **kw):
    coarse = T.counts_from_scores(S, cls, lo, hi)
    return T.calibration_from_passes(coarse, lambda b: T.counts_from_scores(S, cls, lo, hi, 0, T.BINS * b), lambda a, c: T.calib_sums_host(S, cls, a, c),
                                     "plda", lo, hi, **kw)


def test_fit_on_two_gaussians_converges_and_lowers_cllr():
    S, cls = two_gaussians()
    cal = host_calibration(S, cls, -16.0, 16.0)
    theta = math.log(PRIOR / (1 - PRIOR))
    J, g, _ = T.objective(T.calib_sums_host(S, cls, cal.a, cal.b + theta), PRIOR)
    assert cal.converged and (np.abs(g) <= 1e-10 * J).all() and np.allclose(cal.grad, g, rtol=0, atol=1e-16)
    assert cal.cllr <= cal.cllr_raw and 3 <= cal.n_passes <= 26 and (cal.n_target, cal.n_nontarget, cal.n_nonfinite, cal.n_excluded) == (20000, 20000, 0, 0)
    # equal-variance Gaussians at +-1 with variance 1: the true llr is 2 s, and the prior-weighted fit estimates it
    assert abs(cal.a - 2.0) < 0.1 and abs(cal.b) < 0.1
    assert cal.min_cllr_coarse <= cal.cllr + 1e-12 and cal.min_dcf <= cal.act_dcf
    assert cal.bayes_threshold == (-theta - cal.b) / cal.a
    q, _ = CR.quantise(cal.bayes_threshold, -16.0, 16.0)
    assert cal.act_dcf == CR.dcf_at(S, cls, -16.0, 16.0, int(q), 0.01, 1.0, 1.0)
    try:
        from scipy.optimize import minimize
    except ImportError:
        return
    ref = minimize(lambda x: T.objective(T.calib_sums_host(S, cls, x[0], x[1] + theta), PRIOR)[0], [1.0, 0.0], method="BFGS",
                   jac=lambda x: T.objective(T.calib_sums_host(S, cls, x[0], x[1] + theta), PRIOR)[1], options={"gtol": 1e-9})
    # BFGS stops at |grad| <= gtol: its distance from the minimiser is at most ||H^-1|| gtol (a few times that with its own rounding)
    H = T.objective(T.calib_sums_host(S, cls, cal.a, cal.b + theta), PRIOR)[2]
    assert np.abs(ref.x - [cal.a, cal.b]).max() <= 4 * np.linalg.norm(np.linalg.inv(H), 2) * max(1e-9, float(np.abs(ref.jac).max()))


def test_separable_classes_do_not_converge_and_an_empty_class_is_refused():
    rng = np.random.default_rng(4)
    S = np.concatenate([rng.uniform(1.0, 3.0, 500), rng.uniform(-3.0, -1.0, 500)])
    cls = np.concatenate([np.ones(500, np.int64), np.zeros(500, np.int64)])
    cal = host_calibration(S, cls, -4.0, 4.0)
    assert cal.converged is False and cal.n_passes <= 26
    with pytest.raises(ValueError, match="both classes"):
        host_calibration(S[:500], cls[:500], -4.0, 4.0)
    with pytest.raises(ValueError, match="both classes"):
        T.fit_from_counts(T.counts_from_scores(S[:500], cls[:500], -4.0, 4.0), -4.0, 4.0, PRIOR)


def test_the_coarse_start_approaches_the_exact_fit_as_the_range_shrinks():
    S, cls = two_gaussians(5000, seed=6)
    theta = math.log(PRIOR / (1 - PRIOR))
    exact = T.newton_fit(lambda a, c: T.calib_sums_host(S, cls, a, c), 1.0, 0.0, PRIOR, max_passes=60)
    assert exact.converged
    dist = []
    for half in (4096.0, 512.0, 64.0, 8.0):                      # bins of 2, 1/4, 1/32 and 1/256
        start = T.fit_from_counts(T.counts_from_scores(S, cls, -half, half), -half, half, PRIOR)
        dist.append(max(abs(start.a - exact.a), abs(start.b - exact.b)))
    assert dist[0] > dist[1] > dist[2] > dist[3] and dist[3] < 1e-3, dist
    assert theta < 0


# ---- PAV ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_pav_equals_the_textbook_algorithm(seed):
    rng = np.random.default_rng(seed)
    hist = np.zeros((2, T.BINS), np.int64)
    where = np.sort(rng.choice(T.BINS, 60, replace=False))
    ramp = np.linspace(0.05, 0.95, 60)
    hist[1, where] = rng.binomial(40, ramp)
    hist[0, where] = rng.binomial(40, 1 - ramp)
    hist[:, where[10]] = hist[:, where[11]] = (7, 7)             # a tie of two adjacent cells, among empty bins
    hist[:, where[20]] = (0, 9)                                  # targets only
    hist[:, where[21]] = (9, 0)                                  # nontargets only, right after: a violation
    p = T.PassCounts(hist, np.asarray([seed, 2]), np.asarray([1, 3 * seed]), np.zeros(2, np.int64), 0)
    t = [int(p.under[1])] + hist[1].tolist() + [int(p.over[1])]
    n = [int(p.under[0])] + hist[0].tolist() + [int(p.over[0])]
    got, want = T.pav_min_cllr(p), float(CR.pav_min_cllr(t, n))
    assert abs(got - want) <= 1e-13 * want and 0.0 < got < 1.0
    with pytest.raises(ValueError, match="both classes"):
        T.pav_min_cllr(T.PassCounts(np.stack([hist[0], 0 * hist[1]]), np.zeros(2, np.int64), np.zeros(2, np.int64), np.zeros(2, np.int64), 0))


# ---- the file and the environment ----------------------------------------------------------------------------------------------------------
def test_save_load_round_trip_and_refusals(tmp_path):
    S, cls = two_gaussians(2000, seed=9)
    cal = host_calibration(S, cls, -16.0, 16.0)
    path = tmp_path / "cal.json"
    T.save_calibration(cal, path)
    assert T.load_calibration(path) == cal
    doc = json.loads(path.read_text())
    assert set(doc) == set(T.CALIBRATION_KEYS)

    def refused(match, **change):
        bad = tmp_path / "bad.json"
        bad.write_text(json.dumps({**doc, **change}))
        with pytest.raises(ValueError, match=match):
            T.load_calibration(bad)
        return bad

    refused("a > 0", a=0.0)
    refused("a > 0", a=-1.5)
    refused("finite", a=float("nan"))
    refused("finite", b=float("inf"))
    refused("kind", kind="snorm")
    refused("numbers", a="steep")
    refused("prior", prior=0.0)
    refused("prior", prior=1.5)
    refused("score range", score_range=[2.0, 2.0])
    refused("score range", score_range=[0.0, float("inf")])
    # standard JSON: a figure that is not finite is written as null and read back as NaN; a map that would be refused is not written
    hand = T.Calibration(kind="cosine", a=2.0, b=-1.0, prior=PRIOR, score_range=(-2.0, 2.0))
    T.save_calibration(hand, tmp_path / "hand.json")
    text = (tmp_path / "hand.json").read_text()
    assert "NaN" not in text and "Infinity" not in text and json.loads(text, parse_constant=lambda c: pytest.fail(c))["cllr"] is None
    back = T.load_calibration(tmp_path / "hand.json")
    assert (back.kind, back.a, back.b, back.prior, back.score_range, back.converged) == ("cosine", 2.0, -1.0, PRIOR, (-2.0, 2.0), False)
    assert math.isnan(back.cllr) and math.isnan(back.act_dcf) and all(math.isnan(g) for g in back.grad)
    for bad in (dict(a=float("nan")), dict(a=-1.0), dict(kind="snorm"), dict(prior=1.0)):
        with pytest.raises(ValueError):
            T.save_calibration(T.Calibration(**{**dict(kind="cosine", a=2.0, b=-1.0, prior=PRIOR, score_range=(-2.0, 2.0)), **bad}), tmp_path / "never.json")
    assert not (tmp_path / "never.json").exists()
    (tmp_path / "bad.json").write_text(json.dumps({"kind": "cosine"}))
    with pytest.raises(ValueError, match="not a calibration file"):
        T.load_calibration(tmp_path / "bad.json")
    # rule_from_env: every refusal of the setting
    env = {"SDK_SCORE_CALIBRATION": str(path)}
    with pytest.raises(ValueError, match="fitted to the 'plda' rule, the configured rule is 'cosine'"):
        RULES.rule_from_env(env)
    with pytest.raises(ValueError, match="SDK_SCORE_CALIBRATION together with SDK_COHORT"):
        RULES.rule_from_env({**env, "SDK_COHORT": "c.npy", "SDK_COHORT_THRESHOLD": "1"})
    with pytest.raises(ValueError, match="a > 0"):
        RULES.rule_from_env({"SDK_SCORE_CALIBRATION": str(refused("a > 0", a=-2.0))})
    for prior in ("0", "1", "likely"):
        with pytest.raises(ValueError, match="SDK_SCORE_PRIOR"):
            RULES.rule_from_env({**env, "SDK_SCORE_PRIOR": prior})
    rule = RULES.rule_from_env({**env, "SDK_SCORE_PLDA_TRANSFORM": "t.npz", "SDK_SCORE_PLDA": "p.npz", "SDK_SCORE_PRIOR": "0.2"})
    assert rule.kind == "plda" and rule.calibration == cal and rule.score_prior == 0.2 and rule.verify_keys == ("llr", "calibrated_llr", "posterior")
    plain = RULES.rule_from_env({})
    assert plain.calibration is None and plain.verify_keys == () and RULES.Plda.verify_keys == ("llr",)


@pytest.mark.parametrize("kind", ["cosine", "plda"])
def test_rows_gain_exactly_two_keys(tmp_path, kind):
    path = tmp_path / "cal.json"
    T.save_calibration(T.Calibration(kind=kind, a=7.25, b=-1.5, prior=PRIOR, score_range=(-2.0, 2.0)), path)
    env = {"SDK_SCORE_PLDA_TRANSFORM": "t.npz", "SDK_SCORE_PLDA": "p.npz"} if kind == "plda" else {}
    plain, cal = RULES.rule_from_env(env), RULES.rule_from_env({**env, "SDK_SCORE_CALIBRATION": str(path), "SDK_SCORE_PRIOR": "0.25"})
    rng = np.random.default_rng(1)
    idx = rng.integers(-1, 3, 30).astype(np.int32)
    spans = [(float(w), w + 2.0) for w in range(30)]

    class batch:
        speaker_ids, embedding_ids = ["ann", "bob", "ann"], ["e0", "e1", "e2"]

        def __len__(self):
            return 3

    class be:                                                    # what Plda.rows asks of its Backend
        @staticmethod
        def speaker_table(b):
            return None, None, ["ann", "bob"], [0, 1], [2, 1]

    if kind == "cosine":
        cols, key = (idx, rng.uniform(-1, 1, 30).astype(np.float32)), "similarity"
    else:
        cols, key = (np.minimum(idx, 1), rng.normal(0, 5, 30)), "llr"
    want, got = plain.rows(be, cols, spans, batch(), 0.1), cal.rows(be, cols, spans, batch(), 0.1)
    assert len(got) == len(want) > 0
    for w, g in zip(want, got):
        assert list(g)[:len(w)] == list(w) and {k: g[k] for k in w} == w and set(g) - set(w) == {"calibrated_llr", "posterior"}
        llr = float(np.float64(7.25) * np.float64(w[key]) + np.float64(-1.5))
        assert g["calibrated_llr"] == llr and abs(g["posterior"] - 1 / (1 + math.exp(-(llr + math.log(0.25 / 0.75))))) <= 1e-15
    assert plain.rows(be, cols, spans, batch(), 0.1) == want      # the plain rule's rows carry neither key


def test_the_torch_free_path_applies_the_calibration(tmp_path, monkeypatch):
    """SDK_NO_TORCH=1 (the cosine rule only) with SDK_SCORE_CALIBRATION: identify_speaker, identify_many and verify_speaker carry the two keys."""
    BK = sub("backend")
    path = tmp_path / "cal.json"
    T.save_calibration(T.Calibration(kind="cosine", a=7.25, b=-1.5, prior=PRIOR, score_range=(-2.0, 2.0)), path)
    for v in ("SDK_COHORT", "SDK_COHORT_THRESHOLD", "SDK_SCORE_PLDA_TRANSFORM", "SDK_SCORE_PLDA", "SDK_SCORE_PRIOR", "SDK_SCORE_CALIBRATION"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("SDK_NO_TORCH", "1")
    monkeypatch.setenv("SDK_ECAPA_WEIGHTS", "unused.npz")             # only silences the synthetic-weights notice; nothing is loaded here

    class batch:
        speaker_ids, embedding_ids = ["ann", "bob", "ann"], ["e0", "e1", "e2"]

        def __len__(self):
            return 3

    idx = np.asarray([0, 1, 2, 0, -1, 1], np.int32)[:, None]
    cos = np.asarray([0.9, 0.4, 0.8, 0.1, 0.0, 0.6], np.float32)[:, None]

    def stubbed():
        be = BK.Backend()
        assert be.lite
        be._load_candidates = lambda candidates: batch()
        be._windows = lambda p, segments: ("samples", "starts", 32000, [(float(w), w + 2.0) for w in range(6)])
        be.embed_tables_host = lambda samples, tables, b=None, k=1: {32000: (None, idx, cos)}
        return be

    plain = stubbed().identify_speaker("a.wav", [], threshold=0.3)
    plain_verify = stubbed().verify_speaker("a.wav", {}, threshold=0.3)
    monkeypatch.setenv("SDK_SCORE_CALIBRATION", str(path))
    be = stubbed()
    rows = be.identify_speaker("a.wav", [], threshold=0.3)
    assert [r["speaker_id"] for r in plain] == ["ann", "bob"] and len(rows) == 2 and be._engine is None
    for w, g in zip(plain, rows):
        assert {k: g[k] for k in w} == w and list(g)[:len(w)] == list(w) and set(g) - set(w) == {"calibrated_llr", "posterior"}
        assert g["calibrated_llr"] == float(np.float64(7.25) * np.float64(w["similarity"]) + np.float64(-1.5))
        assert abs(g["posterior"] - 1 / (1 + math.exp(-g["calibrated_llr"]))) <= 1e-15
    assert be.identify_many(["a.wav", "b.wav"], []) == [be.identify_speaker("a.wav", [])] * 2
    got = be.verify_speaker("a.wav", {}, threshold=0.3)
    assert {k: got[k] for k in plain_verify} == plain_verify and set(got) - set(plain_verify) == {"calibrated_llr", "posterior"}
    assert (got["calibrated_llr"], got["posterior"]) == (rows[0]["calibrated_llr"], rows[0]["posterior"])
