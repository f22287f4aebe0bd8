"""CPU checks of the PLDA log-likelihood-ratio scoring's host half (plda_score.py, the Backend's configuration) against the independent
references of tests/plda_score_ref.py: Kaldi's direct form and, for a handful of pairs, the joint Gaussian of the model itself."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plda_score_ref as PR  # noqa: E402
from conftest import sub  # noqa: E402

PS = sub("plda_score")
PLDA = sub("plda")
U53 = 2.0 ** -53


def spectrum(D):
    return PLDA.synthetic_plda(192, 128, lda_dim=D).Phi


@pytest.mark.parametrize("D", [64, 128])
def test_restatements_against_the_direct_form(D):
    """speaker_table_host + llr_host against the two log-densities subtracted.  The direct form cancels two sums of D terms of size up to
    (1 + x^2): both sides are good to a few hundred units of 2^-53 of A = |r| + sum |terms| plus the same of the direct form's own terms."""
    rng = np.random.default_rng(D)
    Phi = spectrum(D)
    N, S = 23, 9
    X, Xp, group, counts = PR.planted(rng, N, S, D, Phi)
    n_eff = counts.astype(np.float64)
    n_eff[3] = 2.5                                                       # a non-integer effective count
    n_eff[4], n_eff[5], n_eff[6] = 1.0, 3.0, 7.0
    G, r = PS.speaker_table_host(Xp, group, n_eff, Phi)
    Gr, rr, U, m = PR.table(Xp, group, n_eff, Phi)
    assert G.shape == (S, 2 * D) and r.shape == (S,) and np.array_equal(m, counts)
    assert np.allclose(G, Gr, rtol=1e-13, atol=1e-15) and np.allclose(r, rr, rtol=1e-12, atol=1e-12)
    L = PS.llr_host(X, G, r)
    Ld = PR.llr_direct(X, U, m, n_eff, Phi)
    direct_mag = 0.5 * ((X[:, None, :] - 0.0) ** 2).sum(-1) + 0.5 * (X ** 2).sum(-1)[:, None] + D * 3.0 + np.abs(Ld)
    bound = 4 * (2 * D + 4) * U53 * (PR.magnitude(X, G, r) + direct_mag)
    print(f"D={D}: worst |llr_host - direct| / bound = {float((np.abs(L - Ld) / bound).max()):.4f}")
    assert (np.abs(L - Ld) <= bound).all()
    Lt = PR.llr_table(X, Gr, rr)
    assert (np.abs(L - Lt) <= (2 * D + 4) * U53 * PR.magnitude(X, Gr, rr) * 2).all()
    for k in (1, 3, 4):
        idx, sc = PS.topk_host(L, k)
        ridx, rsc = PR.topk(L, k)
        assert idx.dtype == np.int32 and np.array_equal(idx, ridx) and np.array_equal(sc, rsc)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("n", [1, 3, 7])
def test_score_against_the_joint_gaussian(D, n):
    rng = np.random.default_rng(10 * D + n)
    Phi = spectrum(D)
    for _ in range(3):
        centre = rng.standard_normal(D) * np.sqrt(Phi)
        rows = centre + rng.standard_normal((n, D))
        x = (centre if rng.random() < 0.5 else rng.standard_normal(D) * np.sqrt(Phi)) + rng.standard_normal(D)
        G, r = PS.speaker_table_host(rows, np.zeros(n, np.int32), np.asarray([float(n)]), Phi)
        got = float(PS.llr_host(x[None], G, r)[0, 0])
        want = PR.llr_joint(x, rows, Phi)
        assert abs(got - want) <= 1e-10 * (1.0 + abs(want)), (got, want)


def test_coefficients_shapes_and_symmetry_at_one_enrolment():
    D = 64
    Phi = spectrum(D)
    g, q, h, c = PS.coefficients(Phi, 1.0)
    assert g.shape == q.shape == h.shape == (D,) and np.ndim(c) == 0
    g2, q2, h2, c2 = PS.coefficients(Phi, np.asarray([1.0, 2.5]))
    assert g2.shape == (2, D) and c2.shape == (2,) and np.array_equal(g2[0], g) and c2[0] == c
    assert np.allclose(q, h, rtol=1e-12, atol=1e-16)                      # n = 1: x and u enter alike
    rng = np.random.default_rng(0)
    x, u = rng.standard_normal((2, D)) * np.sqrt(1 + Phi)
    one = np.ones(1)

    def llr(a, b):
        G, r = PS.speaker_table_host(b[None], np.zeros(1, np.int32), one, Phi)
        return float(PS.llr_host(a[None], G, r)[0, 0])
    assert abs(llr(x, u) - llr(u, x)) <= 1e-12 * (1 + abs(llr(x, u)))


def test_table_edge_speakers_and_topk_rules():
    D = 64
    Phi = spectrum(D)
    rng = np.random.default_rng(1)
    Xp = rng.standard_normal((6, D))
    group = np.asarray([2, 0, 2, 7, -1, 3], np.int32)                     # 7 and -1 belong to nobody; speaker 1 has no row
    n_eff = np.asarray([1.0, 1.0, 2.0, 0.0, np.nan])
    G, r = PS.speaker_table_host(Xp, group, n_eff, Phi)
    assert np.isnan(r[[1, 3, 4]]).all() and np.isfinite(r[[0, 2]]).all() and not G[[1, 3, 4]].any()
    Gr, rr, _, _ = PR.table(Xp, group, n_eff, Phi)
    assert np.allclose(G, Gr, rtol=1e-13) and np.allclose(r, rr, rtol=1e-12, equal_nan=True)
    L = np.asarray([[1.0, np.nan, 1.0, -2.0], [np.nan] * 4, [0.0, -0.0, 5.0, 5.0]])
    idx, sc = PS.topk_host(L, 3)
    assert idx.tolist() == [[0, 2, 3], [-1, -1, -1], [2, 3, 0]] and sc[1].tolist() == [0.0, 0.0, 0.0] and sc[0].tolist() == [1.0, 1.0, -2.0]
    idx, sc = PS.topk_host(L[:, :2], 4)                                  # k > S: the columns S .. k - 1 hold (-1, 0)
    assert idx.shape == (3, 4) and idx[0].tolist() == [0, -1, -1, -1] and (idx[:, 2:] == -1).all() and not sc[:, 2:].any()
    with pytest.raises(ValueError):
        PS.topk_host(L, 5)


def test_group_speakers_on_interleaved_ids():
    group, speakers, first, counts = PS.group_speakers(["bob", "ann", "bob", "cy", "ann", "bob"])
    assert group.dtype == np.int32 and group.tolist() == [0, 1, 0, 2, 1, 0]
    assert speakers == ["bob", "ann", "cy"] and first.tolist() == [0, 1, 3] and counts.tolist() == [3, 2, 1]
    group, speakers, first, counts = PS.group_speakers([])
    assert group.shape == (0,) and speakers == [] and first.shape == (0,) and counts.shape == (0,)


def test_aggregation_rule():
    speakers, emb, counts = ["bob", "ann", "cy"], ["e-bob-0", "e-ann-0", "e-cy-0"], [3, 2, 1]
    spans = [(float(i), float(i) + 2.0) for i in range(7)]
    idx = np.asarray([0, 1, 0, 2, -1, 1, 1])
    llr = np.asarray([4.0, 1.5, 2.0, 1.4999999, 9.0, np.nan, 3.5])
    rows = PS.aggregate_matches_plda(idx, llr, spans, speakers, emb, counts, 1.5)          # llr == threshold votes; below, -1 and NaN do not
    assert [r["speaker_id"] for r in rows] == ["bob", "ann"]
    assert rows[0] == {"speaker_id": "bob", "llr": 3.0, "similarity": PS.confidence(3.0), "confidence": PS.confidence(3.0),
                       "embedding_id": "e-bob-0", "n_embeddings": 3, "segment": (0.0, 4.0), "n_segments": 2}
    assert rows[1]["llr"] == 2.5 and rows[1]["n_segments"] == 2 and rows[1]["segment"] == (1.0, 8.0) and rows[1]["embedding_id"] == "e-ann-0"
    # the reference's rule on the batch's own rows: embedding_id is the speaker's FIRST row
    sids = ["bob", "ann", "bob", "cy", "ann", "bob"]
    eids = [f"e{i}" for i in range(6)]
    group, spk, first, cnt = PS.group_speakers(sids)
    got = PS.aggregate_matches_plda(idx, llr, spans, spk, [eids[p] for p in first], cnt, 1.5)
    want = PR.aggregate(idx, llr, spans, sids, eids, 1.5)
    assert got == want and got[0]["embedding_id"] == "e0" and got[1]["embedding_id"] == "e1"
    # equal llr: ordered by speaker id
    tie = PS.aggregate_matches_plda(np.asarray([0, 1]), np.asarray([2.0, 2.0]), spans[:2], speakers, emb, counts, 0.0)
    assert [r["speaker_id"] for r in tie] == ["ann", "bob"]
    # +-800 without overflow
    far = PS.aggregate_matches_plda(np.asarray([0, 1]), np.asarray([800.0, -800.0]), spans[:2], speakers, emb, counts, -1000.0)
    assert far[0]["confidence"] == 1.0 and far[1]["confidence"] == 0.0 and far[0]["similarity"] == far[0]["confidence"]
    assert PS.confidence(0.0) == 0.5 and abs(PS.confidence(-800.0)) == 0.0 and PS.confidence(800.0) == 1.0


SCORE_VARS = ("SDK_SCORE_PLDA_TRANSFORM", "SDK_SCORE_PLDA", "SDK_SCORE_PLDA_DIM", "SDK_SCORE_PLDA_THRESHOLD", "SDK_SCORE_PLDA_COUNT")


def clean(monkeypatch):
    for v in SCORE_VARS + ("SDK_COHORT", "SDK_COHORT_THRESHOLD", "SDK_NO_TORCH"):
        monkeypatch.delenv(v, raising=False)


def test_backend_refusals_touch_no_device(monkeypatch, tmp_path):
    BK = sub("backend")
    clean(monkeypatch)
    t, p = str(tmp_path / "xvec_transform.npz"), str(tmp_path / "plda.npz")
    monkeypatch.setenv("SDK_SCORE_PLDA_TRANSFORM", t)
    with pytest.raises(ValueError, match="SDK_SCORE_PLDA is not set"):
        BK.Backend()
    monkeypatch.delenv("SDK_SCORE_PLDA_TRANSFORM")
    monkeypatch.setenv("SDK_SCORE_PLDA", p)
    with pytest.raises(ValueError, match="SDK_SCORE_PLDA_TRANSFORM is not set"):
        BK.Backend()
    monkeypatch.setenv("SDK_SCORE_PLDA_TRANSFORM", t)
    monkeypatch.setenv("SDK_COHORT", str(tmp_path / "cohort.npy"))
    monkeypatch.setenv("SDK_COHORT_THRESHOLD", "0")
    with pytest.raises(ValueError, match="together with SDK_COHORT"):
        BK.Backend()
    monkeypatch.delenv("SDK_COHORT")
    monkeypatch.delenv("SDK_COHORT_THRESHOLD")
    monkeypatch.setenv("SDK_NO_TORCH", "1")
    with pytest.raises(ValueError, match="SDK_NO_TORCH=1"):
        BK.Backend()
    monkeypatch.delenv("SDK_NO_TORCH")
    for var, bad, what in (("SDK_SCORE_PLDA_DIM", "96", "64 or 128"), ("SDK_SCORE_PLDA_THRESHOLD", "nan", "NaN"),
                           ("SDK_SCORE_PLDA_THRESHOLD", "high", "a float"), ("SDK_SCORE_PLDA_COUNT", "2", "SDK_SCORE_PLDA_COUNT")):
        monkeypatch.setenv(var, bad)
        with pytest.raises(ValueError, match=what):
            BK.Backend()
        monkeypatch.delenv(var)
    monkeypatch.setenv("SDK_SCORE_PLDA_THRESHOLD", "-2.5")
    monkeypatch.setenv("SDK_SCORE_PLDA_COUNT", "0")
    monkeypatch.setenv("SDK_SCORE_PLDA_DIM", "64")
    be = BK.Backend()                                                    # the files are read at first use, not here
    assert be.plda_scoring and be.score_plda_threshold == -2.5 and be.score_plda_count is False and be.score_plda_dim == 64
    assert be._engine is None
    # a model of another width is refused at first use, naming both
    PLDA.save_plda(PLDA.synthetic_plda(256, 128), t, p)
    monkeypatch.setenv("SDK_SCORE_PLDA_DIM", "128")
    be = BK.Backend()
    with pytest.raises(ValueError, match=r"d_in=256.*embedding_dim=192"):
        be.score_plda()
    assert be._engine is None


def test_backend_without_the_variables_reports_no_plda_scoring(monkeypatch):
    BK = sub("backend")
    clean(monkeypatch)
    be = BK.Backend()
    assert be.plda_scoring is False and be.score_plda() is None and be.score_plda_threshold == 0.0 and be._engine is None
    with pytest.raises(ValueError, match="no scoring model configured"):
        be.score_windows_plda(None, None)


def test_symbols_are_declared_and_bound():
    LIB = sub("_lib")
    header = (LIB._HERE.parent / "include" / "sdk_hip.h").read_text()
    for name in ("sdk_plda_enroll_workspace_bytes", "sdk_plda_enroll", "sdk_plda_score_workspace_bytes", "sdk_plda_score_topk"):
        assert name in LIB.SIGNATURES and f"{name}(" in header
    assert "sdk_plda_score_topk" in header.split("BUILDING BLOCKS AND KNOBS")[0]              # listed in the stable surface
