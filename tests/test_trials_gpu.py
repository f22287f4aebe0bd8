"""GPU checks of the verification-trial histogram (sdk_trial_hist, Engine.trial_hist), of trials.evaluate and of Backend.tune_verification.

Bit-exact cases.  Entries of A, B and r that are multiples of 2^-6 of magnitude <= 2: every product is a multiple of 2^-12 and every partial
sum stays below 2^11, so every partial sum is exact in float64 in any order and the device's score equals numpy's bit for bit.  All 8199
counters must then equal trials.trial_hist_host.

The sandwich for rounded inputs.  A score is r_j + sum of K products.  In the kernel a term meets no rounding of its product (the MFMA fuses
it) and the additions of its chain - K of them with the first onto a zero accumulator exact, so K - 1 - and the epilogue's addition of r_j:
K roundings, whatever the order of the chain: gamma_K a <= (K + 1) u a with u = 2^-53 and a(i, j) = |r_j| + sum_k |A_ik B_jk|.  The host
reference is the product in extended precision (64-bit significand: its own error is below K 2^-64 a) rounded once to float64: u a more.
So |device - reference| <= delta = (K + 3) u a (the bound of tests/test_plda_score_gpu.py for a chain without the squares).  q is
non-decreasing in the score, so q(s - delta) <= q(device) <= q(s + delta) for every trial, and for every coarse edge and class the device's
cumulative count lies between the host's count of q(s + delta) < edge and its count of q(s - delta) < edge.  t* is non-decreasing when every
score rises, so the device's t* lies between those of the two perturbed host sets.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trials_ref as TR  # noqa: E402
from conftest import ROOT, sub  # noqa: E402

pytestmark = pytest.mark.gpu

T = sub("trials")
PLDA = sub("plda")
U53 = 2.0 ** -53
assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "the sandwich's host reference needs an extended-precision long double"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_hist(engine, A, B, r, la, sa, lb, sb, lo, hi, shift=12, base=0, max_blocks=0):
    out = engine.trial_hist(dev(A), dev(B), dev(r), dev(la.astype(np.int32)), dev(sa.astype(np.int32)), dev(lb.astype(np.int32)),
                            dev(sb.astype(np.int32)), lo, hi, shift=shift, base=base, max_blocks=max_blocks)
    torch.cuda.synchronize()
    return T.counts_to_host(out)


def same(p, w):
    return (np.array_equal(p.hist, w.hist) and np.array_equal(p.under, w.under) and np.array_equal(p.over, w.over)
            and np.array_equal(p.nan, w.nan) and p.excluded == w.excluded)


def grid_inputs(N, M, K, seed):
    rng = np.random.default_rng(seed)
    A = rng.integers(-128, 129, (N, K)) / 64.0
    B = rng.integers(-128, 129, (M, K)) / 64.0
    r = rng.integers(-128, 129, M) / 64.0
    la, lb = rng.integers(-1, 5, N), rng.integers(-1, 5, M)
    sa, sb = rng.integers(-1, 4, N), rng.integers(-1, 4, M)
    return A, B, r, la, sa, lb, sb


# ---- bit-exact histograms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,K,max_blocks", [(1, 1, 16, 0), (63, 65, 16, 0), (64, 64, 192, 0), (130, 200, 256, 0), (130, 200, 256, 1)])
def test_histograms_are_bit_exact_on_exact_inputs(engine, N, M, K, max_blocks):
    A, B, r, la, sa, lb, sb = grid_inputs(N, M, K, 100 + N + K)
    if N == 1:
        la[:], lb[:], sa[:], sb[:] = 2, 2, 0, 1
    lo, hi = -64.0, 64.0
    want = T.trial_hist_host(A, B, r, la, sa, lb, sb, lo, hi)
    got = gpu_hist(engine, A, B, r, la, sa, lb, sb, lo, hi, max_blocks=max_blocks)
    assert got.total() + int(got.nan.sum()) + got.excluded == N * M
    assert same(got, want)
    b = int(np.argmax(want.hist.sum(axis=0)))
    wantz = T.trial_hist_host(A, B, r, la, sa, lb, sb, lo, hi, 0, 4096 * b)
    gotz = gpu_hist(engine, A, B, r, la, sa, lb, sb, lo, hi, 0, 4096 * b, max_blocks=max_blocks)
    assert gotz.total() == got.total() and int(gotz.hist.sum()) == int(want.hist[:, b].sum()) > 0
    assert same(gotz, wantz)


# ---- rounded inputs: the sandwich --------------------------------------------------------------------------------------------------------
def reference_and_delta(A, B, r):
    """(the product in extended precision rounded once to float64, delta) - the module docstring's bound."""
    K = A.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        S = (A.astype(np.longdouble) @ B.T.astype(np.longdouble) + r.astype(np.longdouble)[None, :]).astype(np.float64)
        mag = np.abs(A) @ np.abs(B).T + np.abs(r)[None, :]
    return S, (K + 3) * U53 * mag * (1 + 2.0 ** -40)


def check_sandwich(engine, A, B, r, la, sa, lb, sb, lo, hi):
    S, delta = reference_and_delta(A, B, r)
    cls = TR.classes(la, sa, lb, sb)
    got = gpu_hist(engine, A, B, r, la, sa, lb, sb, lo, hi)
    q_hi, nan = TR.quantise(S + delta, lo, hi)
    q_lo, _ = TR.quantise(S - delta, lo, hi)
    edges = 4096 * np.arange(4097)
    for c in (0, 1):
        live = (cls == c) & ~nan
        cum = int(got.under[c]) + np.concatenate([[0], np.cumsum(got.hist[c])])
        at_least = np.searchsorted(np.sort(q_hi[live]), edges, side="left")       # trials certainly below the edge
        at_most = np.searchsorted(np.sort(q_lo[live]), edges, side="left")
        assert (at_least <= cum).all() and (cum <= at_most).all()
        assert int(got.nan[c]) == int(((cls == c) & nan).sum())
        assert cum[-1] + int(got.over[c]) == int(live.sum())
    res = T.result_from_passes(got, lambda b: gpu_hist(engine, A, B, r, la, sa, lb, sb, lo, hi, 0, 4096 * b), "cosine", lo, hi)
    t_lo, t_hi = TR.metrics(S - delta, cls, lo, hi)["t_star"], TR.metrics(S + delta, cls, lo, hi)["t_star"]
    assert t_lo <= res.t_star <= t_hi
    scale = T.scale_of(lo, hi)
    assert lo + t_lo / scale <= res.eer_threshold <= lo + t_hi / scale
    print(f"sandwich K={A.shape[1]}: worst delta {float(np.nanmax(delta)):.3e}, t* in [{t_lo}, {t_hi}] -> {res.t_star}, eer {res.eer:.4f}")


def test_unit_rows_inside_the_sandwich(engine):
    rng = np.random.default_rng(11)
    N, M, K, nspk = 150, 170, 192, 6
    centres = rng.standard_normal((nspk, K))
    la, lb = rng.integers(0, nspk, N), rng.integers(0, nspk, M)
    unit = lambda X: (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)        # noqa: E731
    A, B = unit(centres[la] + 1.5 * rng.standard_normal((N, K))), unit(centres[lb] + 1.5 * rng.standard_normal((M, K)))
    sa, sb = rng.integers(-1, 5, N), rng.integers(-1, 5, M)
    check_sandwich(engine, A, B, np.zeros(M), la, sa, lb, sb, *T.COSINE_RANGE)


@pytest.mark.parametrize("D", [64, 128])
def test_a_plda_enroll_table_inside_the_sandwich(engine, D):
    rng = np.random.default_rng(12 + D)
    model = PLDA.synthetic_plda(192, 128, lda_dim=D)
    S, P, N = 9, 40, 140
    spk = np.sqrt(model.Phi)[None, :] * rng.standard_normal((S, D))
    group = rng.integers(0, S - 1, P).astype(np.int32)                      # the last speaker has no row: r = NaN
    Xp = spk[group] + rng.standard_normal((P, D))
    la = rng.integers(-1, S, N)
    X = spk[np.maximum(la, 0)] + rng.standard_normal((N, D))
    n_eff = np.bincount(group, minlength=S).astype(np.float64)
    G, r, status = engine.plda_enroll(dev(Xp), dev(group), dev(n_eff), dev(model.Phi))
    Xd = dev(X)
    A = torch.cat([Xd, Xd * Xd], dim=1).cpu().numpy()
    G, r = G.cpu().numpy(), r.cpu().numpy()
    assert int(status.item()) == 0 and np.isnan(r[S - 1]) and np.isfinite(r[:S - 1]).all()
    check_sandwich(engine, A, G, r, la, rng.integers(-1, 3, N), np.arange(S), np.full(S, -1), *T.PLDA_RANGE)


# ---- edges ---------------------------------------------------------------------------------------------------------------------------------
def test_labels_sessions_and_special_scores(engine):
    K = 16
    A = np.zeros((5, K))
    A[:, 0] = [1.0, 0.5, 0.25, -1.0, 2.0]
    B = np.zeros((6, K))
    B[:, 0] = 1.0
    r = np.asarray([0.0, np.nan, np.inf, -np.inf, 1.0, -3.0])
    la, sa = np.asarray([0, 1, -1, 2, 0]), np.asarray([7, -1, 3, 4, -1])
    lb, sb = np.asarray([0, 1, 0, 2, -5, 0]), np.asarray([7, -1, 9, 9, 9, -1])
    lo, hi = -1.0, 3.0                       # scale = 2^22
    want = T.trial_hist_host(A, B, r, la, sa, lb, sb, lo, hi)
    got = gpu_hist(engine, A, B, r, la, sa, lb, sb, lo, hi)
    assert same(got, want)
    # by hand: excluded = row 2 (label -1: 6) + column 4 (label -5: the 4 other rows) + (row 0, column 0): the same session 7
    assert got.excluded == 6 + 4 + 1
    # session -1 on both sides (row 1 x column 1, row 4 x column 5) is NOT excluded: (1, 1) is a NaN target, (4, 5) is a target at 2 - 3 = lo
    assert got.nan.tolist() == [3, 1]        # column 1 (r = NaN): rows 0, 3, 4 nontarget, row 1 target
    assert got.over.tolist() == [2, 2]       # column 2 (r = +inf, label 0): rows 1, 3 nontarget, rows 0, 4 target
    assert got.under.tolist() == [5, 2]      # column 3 (r = -inf, label 2): rows 0, 1, 4 / row 3; column 5 (r = -3): rows 1, 3 / row 0 below lo
    assert got.hist[1][0] == 1 and got.hist[0][0] == 1                        # (4, 5) a target exactly at lo; (3, 0) a nontarget exactly at lo
    assert got.total() + int(got.nan.sum()) + got.excluded == 30
    # a score exactly at hi is above: with hi = 2, (4, 0) has s = 2 and joins the two +inf targets
    got2 = gpu_hist(engine, A, B, r, la, sa, lb, sb, -2.0, 2.0)
    assert same(got2, T.trial_hist_host(A, B, r, la, sa, lb, sb, -2.0, 2.0)) and got2.over.tolist() == [2, 3]


def test_every_trial_excluded_and_bases_that_leave_nothing_in_range(engine):
    A, B, r, la, sa, lb, sb = grid_inputs(70, 66, 32, 5)
    none = gpu_hist(engine, A, B, r, np.full(70, -1), sa, lb, sb, -64.0, 64.0)
    assert none.excluded == 70 * 66 and none.total() == 0 and none.nan.sum() == 0
    one_session = gpu_hist(engine, A, B, r, la, np.zeros(70, int), lb, np.zeros(66, int), -64.0, 64.0)
    assert one_session.excluded == 70 * 66
    for shift, base in ((12, 4096), (0, 1 << 24), (24, 1), (24, 0)):
        got = gpu_hist(engine, A, B, r, la, sa, lb, sb, -64.0, 64.0, shift, base)
        assert same(got, T.trial_hist_host(A, B, r, la, sa, lb, sb, -64.0, 64.0, shift, base))
        if base:
            assert got.hist.sum() == 0 and got.under.sum() > 0               # everything is under (or above the range: over)
    tiny = gpu_hist(engine, A, B, r, la, sa, lb, sb, 1000.0, 1001.0)           # the whole set lies below the range
    assert tiny.hist.sum() == 0 and tiny.over.sum() == 0 and tiny.under.sum() == tiny.total() > 0
    high = gpu_hist(engine, A, B, r, la, sa, lb, sb, -1001.0, -1000.0)
    assert high.hist.sum() == 0 and high.under.sum() == 0 and high.over.sum() == high.total() > 0


def test_refusals(engine):
    A, B, r, la, sa, lb, sb = grid_inputs(8, 8, 32, 6)
    d = [dev(A), dev(B), dev(r)] + [dev(x.astype(np.int32)) for x in (la, sa, lb, sb)]
    out = torch.zeros(8199, dtype=torch.int64, device="cuda")
    lib, ctx = engine.lib, engine.ctx

    def raw(K=32, N=8, M=8, lo=-1.0, scale=2.0 ** 23, shift=12, base=0, max_blocks=0, A_=d[0]):
        return lib.sdk_trial_hist(ctx, A_.data_ptr() if A_ is not None else None, N, d[1].data_ptr(), d[2].data_ptr(), M, K, d[3].data_ptr(),
                                  d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), lo, scale, shift, base, max_blocks, out.data_ptr(), None)

    assert raw() == 0
    for kw in (dict(K=24), dict(K=528), dict(K=0), dict(shift=25), dict(shift=-1), dict(base=-1), dict(base=(1 << 24) + 1), dict(N=0),
               dict(M=(1 << 20) + 1), dict(scale=float("inf")), dict(scale=float("nan")), dict(scale=0.0), dict(scale=-1.0),      # lo >= hi
               dict(lo=float("nan")), dict(lo=float("-inf")), dict(max_blocks=-1), dict(A_=None)):
        assert raw(**kw) == 2, kw
        assert b"sdk_trial_hist" in lib.sdk_last_error()
    torch.cuda.synchronize()

    def eng(A_=d[0], B_=d[1], lo=-1.0, hi=1.0, **kw):
        return engine.trial_hist(A_, B_, d[2], d[3], d[4], d[5], d[6], lo, hi, **kw)

    wide = torch.zeros((8, 528), dtype=torch.float64, device="cuda")
    odd = torch.zeros((8, 24), dtype=torch.float64, device="cuda")
    for call in (lambda: eng(A_=odd, B_=odd), lambda: eng(A_=wide, B_=wide), lambda: eng(shift=25), lambda: eng(lo=1.0, hi=1.0),
                 lambda: eng(lo=2.0, hi=1.0), lambda: eng(lo=-1e308, hi=1e308), lambda: eng(hi=float("inf")), lambda: eng(lo=float("nan")),
                 lambda: eng(base=-1), lambda: eng(A_=d[0].float()), lambda: eng(A_=d[0].cpu())):
        with pytest.raises(ValueError):
            call()


def test_two_calls_return_identical_counters(engine):
    A, B, r, la, sa, lb, sb = grid_inputs(300, 260, 64, 7)
    A, B = A + 1e-3 * np.random.default_rng(1).standard_normal(A.shape), B * (1 + 2.0 ** -30)       # rounded inputs
    runs = [gpu_hist(engine, A, B, r, la, sa, lb, sb, -40.0, 40.0, max_blocks=mb) for mb in (0, 0, 3)]
    assert same(runs[0], runs[1]) and same(runs[0], runs[2])


# ---- trials.evaluate end to end --------------------------------------------------------------------------------------------------------------
def generated(seed=21, N=300, P=200, d=192, nspk=10):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((nspk, d))
    la, lb = np.arange(N) % nspk, np.arange(P) % nspk
    unit = lambda X: (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)        # noqa: E731
    return (unit(centres[la] + 2.0 * rng.standard_normal((N, d))), la, np.arange(N) % 7,
            unit(centres[lb] + 2.0 * rng.standard_normal((P, d))), lb, np.where(np.arange(P) % 3 == 0, -1, np.arange(P) % 7))


def assert_unambiguous(S, delta, cls, lo, hi):
    """No scored trial lies within delta of a cell edge of the q scale: then q(device) = q(S) for every trial, and the device's metrics
    must EQUAL the brute force on S.  A fact of the seeded inputs (for cosine checked on the host alone)."""
    q_lo, nan = TR.quantise(S - delta, lo, hi)
    q_hi, _ = TR.quantise(S + delta, lo, hi)
    live = (cls >= 0) & ~nan
    assert np.array_equal(q_lo[live], q_hi[live])


def test_evaluate_cosine_equals_the_brute_force(engine):
    Et, la, sa, Em, lb, sb = generated()
    res = T.evaluate(engine, dev(Et), la, sa, dev(Em), lb, sb, kind="cosine", max_refine=4096)
    A, B = Et.astype(np.float64), Em.astype(np.float64)
    S, delta = reference_and_delta(A, B, np.zeros(len(B)))
    cls = TR.classes(la, sa, lb, sb)
    assert_unambiguous(S, delta, cls, *T.COSINE_RANGE)
    ref = TR.metrics(S, cls, *T.COSINE_RANGE)
    assert (res.n_target, res.n_nontarget, res.n_nan, res.n_excluded) == (ref["T"], ref["Nn"], 0, ref["n_excluded"])
    assert res.n_excluded > 0 and res.n_target + res.n_nontarget + res.n_excluded == 300 * 200 and (res.test_rows, res.model_rows) == (300, 200)
    assert res.eer == ref["eer"] and res.eer_threshold == ref["eer_threshold"] and res.min_dcf == ref["min_dcf"] and res.min_dcf_exact
    assert res.kind == "cosine" and res.score_range == T.COSINE_RANGE and 0.0 < res.eer < 0.5
    print(f"evaluate cosine: eer {res.eer:.4f} at {res.eer_threshold:.4f}, min_dcf {res.min_dcf:.4f} at {res.min_dcf_threshold:.4f}, {res.n_zooms} zooms")


@pytest.mark.parametrize("by_book", [True, False])
def test_evaluate_plda_equals_the_brute_force_on_the_devices_own_scores(engine, by_book):
    Et, la, sa, Em, lb, sb = generated(seed=22)
    lb = lb.copy()
    lb[5] = -1                                                             # a model row without a speaker is not enrolled
    model = PLDA.synthetic_plda(192, 128, seed=3)
    res = T.evaluate(engine, dev(Et), la, sa, dev(Em), lb, sb, kind="plda", plda=model, count_by_book=by_book, max_refine=4096)
    G, r, spk, sess = T.plda_model_rows(engine, dev(Em), lb, sb, model, by_book)
    A = T.plda_test_rows(engine, dev(Et), model)
    D = model.lda_dim
    _, _, full = engine.plda_score_topk(A[:, :D].contiguous(), G, r, k=1, scores=True)
    torch.cuda.synchronize()
    S = full.cpu().numpy()
    An, Gn, rn = A.cpu().numpy(), G.cpu().numpy(), r.cpu().numpy()
    mag = np.abs(An) @ np.abs(Gn).T + np.abs(rn)[None, :]
    delta = 2 * (2 * D + 4) * U53 * mag                                    # both kernels lie within (2 D + 4) u a of the exact score
    cls = TR.classes(la, sa, spk, sess)
    assert spk.tolist() == list(range(10)) and (sess == -1).all() and cls.shape == (300, 10)
    assert_unambiguous(S, delta, cls, *T.PLDA_RANGE)
    ref = TR.metrics(S, cls, *T.PLDA_RANGE)
    assert (res.n_target, res.n_nontarget, res.n_nan, res.n_excluded) == (ref["T"], ref["Nn"], 0, 0) and res.n_target == 300
    assert res.eer == ref["eer"] and res.eer_threshold == ref["eer_threshold"] and res.min_dcf == ref["min_dcf"] and res.min_dcf_exact
    assert res.kind == "plda" and res.score_range == T.PLDA_RANGE and (res.test_rows, res.model_rows) == (300, 10)
    print(f"evaluate plda by_book={by_book}: eer {res.eer:.4f} at {res.eer_threshold:.3f}, min_dcf {res.min_dcf:.4f} at {res.min_dcf_threshold:.3f}")


# ---- the Backend ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cosine", "plda"])
def test_backend_tune_verification(tmp_path, monkeypatch, kind):
    sys.path.insert(0, str(ROOT / "evals"))
    from run_eval import render_voice
    wav, BK = sub("wav"), sub("backend")
    monkeypatch.setenv("SPEAKERS_EMBEDDINGS_DIR", str(tmp_path / "store"))
    monkeypatch.setenv("SDK_CACHE_DIR", str(tmp_path / "cache"))
    for v in ("SDK_COHORT", "SDK_COHORT_THRESHOLD", "SDK_NO_TORCH", "SDK_SCORE_PLDA_DIM", "SDK_SCORE_PLDA_THRESHOLD", "SDK_SCORE_PLDA_COUNT",
              "SDK_SCORE_PLDA_TRANSFORM", "SDK_SCORE_PLDA"):
        monkeypatch.delenv(v, raising=False)
    if kind == "plda":
        tnpz, pnpz = tmp_path / "xvec_transform.npz", tmp_path / "plda.npz"
        monkeypatch.setenv("SDK_SCORE_PLDA_TRANSFORM", str(tnpz))
        monkeypatch.setenv("SDK_SCORE_PLDA", str(pnpz))
    be = BK.Backend()
    if kind == "plda":
        PLDA.save_plda(PLDA.synthetic_plda(be.embedding_dim, 128), tnpz, pnpz)

    def recording(name, tag, seconds, seed):
        path = tmp_path / f"{name}.wav"
        wav.write_wav_s16(path, render_voice(tag, seconds, seed))
        return path

    profiles = []
    for i, (sid, takes) in enumerate((("ann", 2), ("bob", 1), ("cy", 1))):
        embs = []
        for t in range(takes):
            rec = be.enroll_speaker(recording(f"enroll_{sid}_{t}", sid, 5.0, 100 + 7 * i + 50 * t))
            embs.append({"id": f"emb-{sid}-{t}", "external_id": rec["external_id"], "model_version": rec["model_version"], "trust_level": "high"})
        profiles.append({"id": sid, "names": {"default": sid.title()}, "embeddings": {"mi355x": embs}})
    paths = [recording(f"dev_{j}", tag, 4.0, 300 + j) for j, tag in enumerate(("ann", "bob", "cy", "stranger"))]
    ids = ["ann", "bob", "cy", "nobody-enrolled"]
    out = be.tune_verification(paths, ids, profiles)
    assert {"kind", "eer", "eer_threshold", "min_dcf", "min_dcf_threshold", "min_dcf_lower", "min_dcf_exact", "n_target", "n_nontarget", "n_nan",
            "n_excluded", "n_test_rows", "n_model_rows", "score_range", "result"} == set(out)
    lo, hi = out["score_range"]
    assert out["kind"] == kind and (lo, hi) == (T.COSINE_RANGE if kind == "cosine" else T.PLDA_RANGE)
    assert np.isfinite(out["eer_threshold"]) and lo <= out["eer_threshold"] <= hi
    assert np.isfinite(out["min_dcf_threshold"]) and lo <= out["min_dcf_threshold"] <= hi
    assert 0.0 <= out["eer"] <= 1.0 and out["min_dcf_lower"] <= out["min_dcf"]
    windows = sum(len(be._windows(p, None)[3]) for p in paths)
    assert out["n_test_rows"] == windows and out["n_model_rows"] == (4 if kind == "cosine" else 3)
    assert out["n_target"] + out["n_nontarget"] + out["n_nan"] + out["n_excluded"] == windows * out["n_model_rows"]
    assert out["n_excluded"] == 0 and out["n_nan"] == 0 and out["n_target"] > 0 and out["n_nontarget"] > 0
    res = be.score_verification(paths, ids, profiles)
    assert same(res.counts, out["result"].counts) and res.eer == out["eer"]
    print(f"tune_verification {kind}: {out['n_test_rows']} windows x {out['n_model_rows']} model rows, eer {out['eer']:.4f} at "
          f"{out['eer_threshold']:.4f}, min_dcf {out['min_dcf']:.4f} at {out['min_dcf_threshold']:.4f}")
    monkeypatch.setenv("SDK_COHORT", str(tmp_path / "cohort.npy"))
    monkeypatch.setenv("SDK_COHORT_THRESHOLD", "1.0")
    for v in ("SDK_SCORE_PLDA_TRANSFORM", "SDK_SCORE_PLDA"):
        monkeypatch.delenv(v, raising=False)
    with pytest.raises(ValueError, match="AS-norm trials are not built"):
        BK.Backend().tune_verification(paths, ids, profiles)
