"""CPU checks of the PLDA training rule (plda.fit_host, plda.fit_from_stats, plda.save_plda) against the loop-form reference of
tests/plda_fit_ref.py.  Tolerances as in tests/test_plda_fit_gpu.py: per quantity, 8 x the larger distance of the float64 reference to its
long-double and reversed-order runs (after the same host solve), + 4 ulp of the largest magnitude."""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plda_fit_ref as FR  # noqa: E402

PKG = "speaker-diarization-toolkit_amd"
P = importlib.import_module(f"{PKG}.plda")
MARGIN, ULPS = 8.0, 4.0
N, D_IN, D0, LDA_DIM, K, ITERS = 400, 64, 64, 64, 75, 8
_cache = {}


def fixture():
    if not _cache:
        E, lab, planted = FR.labelled_rows(3, N, D_IN, K, unused=(4,), singles=(0, 9))
        runs = {}
        for name, dt, rev in (("f64", np.float64, False), ("ld", np.longdouble, False), ("rev", np.float64, True)):
            model, f = P.fit_from_stats(
                FR.stats(E, None, 0, dt, rev, scatter=False)["total"],
                lambda mean1: FR.stats(FR.stage1_rows(E, mean1, dt), lab, K, dt, rev),
                lambda mean1, lda, mean2: FR.stats(FR.project(E, mean1, lda, mean2, dt), lab, K, dt, rev), N, D0, LDA_DIM, ITERS)
            runs[name] = dict(model=model, fit=f, Phi=model.Phi, objf=f.objf, W=f.W, B=f.B, s1=f.stats1["scatter"], s2=f.stats2["scatter"],
                              sums1=f.stats1["sums"], sums2=f.stats2["sums"])
        _cache.update(E=E, lab=lab, runs=runs, host=P.fit_host(E, lab, D0, LDA_DIM, ITERS, K=K))
    return _cache


def yardstick(runs, q):
    a = np.asarray(runs["f64"][q]).astype(np.longdouble)
    return max(float(np.abs(a - np.asarray(runs[o][q]).astype(np.longdouble)).max()) for o in ("ld", "rev"))


def tolerance(runs, q):
    return MARGIN * yardstick(runs, q) + ULPS * float(np.spacing(np.abs(runs["f64"][q]).max()))


def test_fit_host_against_the_loop_reference():
    fx = fixture()
    runs, (model, f) = fx["runs"], fx["host"]
    ref = runs["f64"]
    assert np.array_equal(f.counts, ref["fit"].counts) and f.n_classes == K - 1 and f.counts[4] == 0 and f.counts[0] == 1
    have = dict(Phi=model.Phi, objf=f.objf, W=f.W, B=f.B, s1=f.stats1["scatter"], s2=f.stats2["scatter"], sums1=f.stats1["sums"], sums2=f.stats2["sums"])
    for q, v in have.items():
        err = float(np.abs(v - ref[q]).max())
        print(f"{q:6s} max|d| {err:.3e}  yardstick {yardstick(runs, q):.3e}  tolerance {tolerance(runs, q):.3e}")
        assert err <= tolerance(runs, q), q
    assert model.lda.shape == (D_IN, D0) and model.tr.shape == (D0, D0) and (np.diff(model.psi) <= 0).all() and model.psi.min() > 1e-12
    assert f.objf.shape == (ITERS,) and f.eigenvalues.shape == (D_IN,) and (np.diff(f.eigenvalues) <= 0).all()


def test_prepare_reproduces_the_em_covariances():
    """W = inv(tr^T tr) and B = inv((tr^T / psi) tr), as prepare forms them, within the yardstick rule."""
    fx = fixture()
    model, f = fx["host"]
    W = np.linalg.inv(model.tr.T @ model.tr)
    B = np.linalg.inv((model.tr.T / model.psi) @ model.tr)
    for q, have, want in (("W", W, f.W), ("B", B, f.B)):
        err = float(np.abs(have - want).max())
        print(f"{q} max|d| {err:.3e}  tolerance {tolerance(fx['runs'], q):.3e}")
        assert err <= tolerance(fx["runs"], q), q
    Phi, T = P.prepare(model.tr, model.psi, LDA_DIM)
    assert np.array_equal(Phi, model.Phi) and np.array_equal(T, model.T)
    # Phi solves B v = Phi W v with the EM's own W and B
    lam = np.sort(np.linalg.eigvals(np.linalg.solve(f.W, f.B)).real)[::-1][:LDA_DIM]
    assert np.abs(lam - Phi).max() <= tolerance(fx["runs"], "Phi") + 1e-9 * Phi.max()


def test_the_objective_never_falls():
    fx = fixture()
    objf = fx["host"][1].objf
    y = yardstick(fx["runs"], "objf")
    print(f"objf {objf.tolist()}  yardstick {y:.3e}")
    assert np.isfinite(objf).all() and (np.diff(objf) >= -y).all() and objf[-1] > objf[0]


def test_relabelling_the_classes_leaves_phi():
    fx = fixture()
    perm = np.random.default_rng(1).permutation(K)
    model, f = P.fit_host(fx["E"], perm[fx["lab"]].astype(np.int32), D0, LDA_DIM, ITERS, K=K)
    err = float(np.abs(model.Phi - fx["host"][0].Phi).max())
    print(f"Phi under a class permutation: max|d| {err:.3e}  tolerance {tolerance(fx['runs'], 'Phi'):.3e}")
    assert err <= tolerance(fx["runs"], "Phi")
    assert np.array_equal(f.counts[perm], fx["host"][1].counts)


def test_every_refusal_raises():
    fx = fixture()
    E, lab = fx["E"], fx["lab"]
    bad = lab.copy()
    bad[3] = -1
    with pytest.raises(ValueError, match="labels must lie in"):
        P.fit_host(E, bad, D0, LDA_DIM, 2)
    bad[3] = K
    with pytest.raises(ValueError, match="labels must lie in"):
        P.fit_host(E, bad, D0, LDA_DIM, 2, K=K)
    with pytest.raises(ValueError, match="classes with a row"):                      # K' < D0 + 1
        P.fit_host(E, (lab % 64).astype(np.int32), D0, LDA_DIM, 2)
    with pytest.raises(ValueError, match="degrees of freedom"):                       # N - K' < d_in
        P.fit_host(E[:100], np.arange(100, dtype=np.int32) % 70, D0, LDA_DIM, 2)
    for d_bad in (32, 96, 576):
        with pytest.raises(ValueError, match="d_in"):
            P.fit_host(np.zeros((N, d_bad), np.float32), lab, 64, 64, 2)
    with pytest.raises(ValueError, match="D0"):
        P.fit_host(E, lab, 63, 64, 2)
    with pytest.raises(ValueError, match="D0"):
        P.fit_host(E, lab, 65, 64, 2)                                                  # above d_in
    with pytest.raises(ValueError, match="lda_dim"):
        P.fit_host(E, lab, 64, 32, 2)
    with pytest.raises(ValueError, match="within-class scatter"):                      # rows confined to 10 dimensions: Sw is singular
        flat = np.zeros((N, D_IN), np.float32)
        flat[:, :10] = E[:, :10]
        flat[:, 10] = 1.0
        P.fit_host(flat / np.linalg.norm(flat, axis=1, keepdims=True), lab, D0, LDA_DIM, 2, K=K)


def test_save_and_load_round_trip(tmp_path):
    model = fixture()["host"][0]
    a, b = tmp_path / "xvec_transform.npz", tmp_path / "plda.npz"
    P.save_plda(model, a, b)
    back = P.load_plda(a, b, LDA_DIM)
    for k in ("mean1", "lda", "mean2", "mu", "tr", "psi", "Phi", "T"):
        assert np.array_equal(getattr(back, k), getattr(model, k)) and getattr(back, k).dtype == np.float64, k
    odd = tmp_path / "model.transform"                                                 # the paths are taken as given
    P.save_plda(model, odd, tmp_path / "model.plda")
    assert odd.exists() and np.array_equal(P.load_plda(odd, tmp_path / "model.plda", LDA_DIM).tr, model.tr)


# ------------------------------------------------------------------------------------------------ the labelling rule
DH = importlib.import_module(f"{PKG}.diarize_host")
SC = importlib.import_module(f"{PKG}.score")
F = 589


def hand_table():
    """Two chunks at 0 and 1 s of a 12-s recording.  Chunk 0: local 0 alone in frames 0..299, local 1 alone in 300..499, both in 500..588."""
    cls = np.zeros((2, F), np.uint8)
    cls[0, :300], cls[0, 300:500], cls[0, 500:] = 1, 2, 4
    cls[1, :400], cls[1, 400:] = 1, 3
    info = np.zeros((2, 3, 4), np.int32)
    info[..., 3] = 1
    for c in range(2):
        for s in range(3):
            info[c, s, 1] = sum(1 for k in cls[c] if FR.POWERSET[k] == (s,))
    return cls, info, np.array([0, 16000], np.int64)


def masks_of(turns, G):
    merged, names = SC.prepare_reference(turns)
    mask, _ = SC.reference_masks_host(merged, G)
    return mask, names, np.array([[(int(m) >> r) & 1 for m in mask] for r in range(len(names))], bool).reshape(len(names), G)


def test_labelling_rule_on_hand_made_tables():
    cls, info, starts = hand_table()
    G = DH.global_frames(12 * 16000)
    sec = lambda g: (270 * g + 495) / 16000.0  # noqa: E731
    # a covers the first 150 clean frames of (chunk 0, local 0) and b the other 150: a tie, to the lower index (a starts first).  c covers
    # 99 of the 200 clean frames of (chunk 0, local 1): below the half-coverage bar, the row is left out.
    turns = [(0.0, sec(150) - 1e-4, "a"), (sec(150) - 1e-4, sec(300) - 1e-4, "b"), (sec(300) - 1e-4, sec(399) - 1e-4, "c")]
    mask, names, dense = masks_of(turns, G)
    assert names == ["a", "b", "c"]
    train = DH.training_mask(info, F)
    assert train[0] and train[1] and not train[2]                                    # (0, 2) has no clean frame: not a training row
    got = DH.reference_labels(cls, info, starts, mask, len(names))
    want = FR.label_rows(cls, starts, train, dense)
    assert np.array_equal(got, want)
    q1 = (135 - 16000) // 270
    assert dense[0, :150].all() and dense[1, 150:300].all() and dense[2, 300:399].all() and not dense[2, 399:].any()
    assert got[0] == 0, "a tie goes to the lower index"
    assert got[1] == -1, "99 of 200 frames is below the bar"
    # exactly half passes
    mask2, names2, dense2 = masks_of(turns[:2] + [(sec(300) - 1e-4, sec(400) - 1e-4, "c")], G)
    assert DH.reference_labels(cls, info, starts, mask2, 3)[1] == 2
    # chunk 1 maps through g = i - q: its frames 0..399 are global frames -q1 .. -q1 + 399
    turns3 = [(sec(-q1) - 1e-4, sec(-q1 + 400) - 1e-4, "z")]
    mask3, _, dense3 = masks_of(turns3, G)
    got3 = DH.reference_labels(cls, info, starts, mask3, 1)
    assert got3[3] == 0 and got3[5] == -1 and np.array_equal(got3, FR.label_rows(cls, starts, train, dense3))
    # no reference speaker at all
    assert (DH.reference_labels(cls, info, starts, np.zeros(G, np.uint64), 0) == -1).all()


def test_speaker_key_merges_a_speaker_across_recordings():
    """The class numbering of Backend.train_plda, restated: (recording, name) unless speaker_key maps several to one."""
    be = importlib.import_module(f"{PKG}.backend")
    rec = np.array([0, 0, 1, 1, 1], np.int32)
    spk = np.array([0, 1, 0, 1, 0], np.int32)
    names = [["ann", "bob"], ["ann", "cy"]]
    lab, keys = be.plda_classes(rec, spk, names, ["r0", "r1"], None)
    assert lab.tolist() == [0, 1, 2, 3, 2] and keys == [("r0", "ann"), ("r0", "bob"), ("r1", "ann"), ("r1", "cy")]
    lab, keys = be.plda_classes(rec, spk, names, ["r0", "r1"], lambda uri, name: name)
    assert lab.tolist() == [0, 1, 0, 2, 0] and keys == ["ann", "bob", "cy"]
    lab, keys = be.plda_classes(rec, spk, names, None, None)
    assert keys == [(0, "ann"), (0, "bob"), (1, "ann"), (1, "cy")]


# ------------------------------------------------------------------------------------------------ the GPU cases at partly live second columns
def test_the_gpu_cases_at_320_and_448_weigh_the_second_column():
    """What tests/test_plda_fit_gpu.py asserts on the reference alone before it asks the device, at the widths where a thread's second column is
    live for a part of the workgroup only: without the columns 256.. of the rows every compared quantity moves by more than 100 x its tolerance."""
    import partial_width as PW
    import test_plda_fit_gpu as FG                                             # its cases and references; importing it needs no GPU
    stats = [c for c in FG.STATS_CASES if c[1] in PW.WIDTHS]
    proj = [c for c in FG.PROJECTION_CASES if c[1] in PW.WIDTHS]
    assert {c[1] for c in stats} == {c[1] for c in proj} == set(PW.WIDTHS) and any(PW.FIRST < c[2] < c[1] for c in proj)
    for case in stats:
        assert FG.stats_weight(case) > PW.FAR
    for case in proj:
        assert FG.projection_weight(case, *FG.projection_reference(case)) > PW.FAR
