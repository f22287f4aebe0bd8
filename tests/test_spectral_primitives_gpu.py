"""The thin [n, k] device primitives of spectral clustering (csrc/spectral.hip: rows_gram, rows_apply, rows_unit, kmeans_mindist,
kmeans_assign, chol_inverse) and the small shapes of affinity_matvec, against the float64 loop references of tests/spectral_ref.py at
the shapes where such kernels break: n = 1, a block boundary (255 / 256 / 257 rows, 513 = two blocks and one row), k = 1 and k = 32
(the LDS row width), kc = 32, exact ties, zero and NaN rows.

Integer-valued inputs make every fp32 chain exact, so those results must equal the reference bit for bit.  Real-valued inputs are held to
bounds DERIVED from the kernels' arithmetic (u = 2^-24):
  rows_gram       |G - G64| <= 256 u sum_r |x_ra||y_rb| + u |G64|      one fmaf chain of <= 256 terms per block, blocks summed in float64
  rows_apply      |Y - Y64| <= (k + 1) u |scale_i| sum_a |x_ia||r_ac|  k fmaf steps, one multiplication
  rows_unit       |U - U64| <= (k + 4) u                               elements of a unit row are <= 1
  dist2, mindist  |d - d64| <= (k + 3) 2^-23 d64                       a rounded difference squared, k fmaf steps, all terms >= 0
Every test prints its worst error / bound before asserting (profiles/r15_spectral_primitives_parity.txt holds one run's figures; no
bound had to be replaced by a measured one).  Labels must equal the float64 argmin wherever the float64 best-minus-second margin
exceeds twice the dist2 bound; tests/test_spectral_primitives_cpu.py checks that this keeps >= 95 % of the rows of every case."""
import numpy as np
import pytest
import torch

import spectral_ref as sr
from conftest import sub

pytestmark = pytest.mark.gpu

CL = sub("cluster")


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def report(what, case, ratio, extra=""):
    print(f"spectral_primitives {what} {case}: worst err / bound = {ratio:.4f}{extra}")


def worst_ratio(got, want64, bound):
    """max |got - want| / bound over the elements (0 / 0 counts as 0: an exact element with a zero bound is fine)."""
    err = np.abs(got.astype(np.float64) - want64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(r.max())


def exact(got, want64):
    """An fp32 result equal to the float64 reference, value for value."""
    return got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want64)


# ------------------------------------------------------------------ rows_gram
@pytest.mark.parametrize("n,k", sr.NK_CASES)
def test_rows_gram(engine, n, k):
    seed = sr.case_seed(n, k)
    Xi, Yi = sr.int_rows(n, k, seed), sr.int_rows(n, k, seed + 1)
    assert exact(host(engine.rows_gram(dev(Xi), dev(Yi))), sr.gram(Xi, Yi))
    Gs = host(engine.rows_gram(dev(Xi), dev(Xi)))
    assert exact(Gs, sr.gram(Xi, Xi)) and np.array_equal(sr.bits(Gs), sr.bits(Gs.T))
    X, Y = sr.real_rows(n, k, seed + 2), sr.real_rows(n, k, seed + 3)
    G = host(engine.rows_gram(dev(X), dev(Y)))
    G64 = sr.gram(X, Y)
    ratio = worst_ratio(G, G64, sr.gram_bound(X, Y, G64))
    Gx = host(engine.rows_gram(dev(X), dev(X)))
    ratio_s = worst_ratio(Gx, sr.gram(X, X), sr.gram_bound(X, X, sr.gram(X, X)))
    report("rows_gram", f"n={n} k={k}", max(ratio, ratio_s))
    assert ratio <= 1.0 and ratio_s <= 1.0
    assert np.array_equal(sr.bits(Gx), sr.bits(Gx.T)), "X^T X must be exactly symmetric"


# ------------------------------------------------------------------ rows_apply
@pytest.mark.parametrize("n,k", sr.NK_CASES)
def test_rows_apply(engine, n, k):
    seed = sr.case_seed(n, k)
    Xi, Ri, sp = sr.int_rows(n, k, seed), sr.int_rows(k, k, seed + 2), sr.pow2_scale(n, seed + 4)
    assert exact(host(engine.rows_apply(dev(Xi), dev(Ri), dev(sp))), sr.apply(Xi, Ri, sp))
    assert exact(host(engine.rows_apply(dev(Xi), dev(Ri))), sr.apply(Xi, Ri))
    X, R = sr.real_rows(n, k, seed + 5), sr.real_rows(k, k, seed + 6)
    sc = np.random.default_rng(seed + 7).uniform(-2, 2, n).astype(np.float32)
    worst = 0.0
    for scale in (sc, None):
        Y = host(engine.rows_apply(dev(X), dev(R), None if scale is None else dev(scale)))
        worst = max(worst, worst_ratio(Y, sr.apply(X, R, scale), sr.apply_bound(X, R, scale)))
    report("rows_apply", f"n={n} k={k}", worst)
    assert worst <= 1.0


# ------------------------------------------------------------------ rows_unit
@pytest.mark.parametrize("n,k", sr.NK_CASES)
def test_rows_unit(engine, n, k):
    X = sr.real_rows(n, k, sr.case_seed(n, k) + 8)
    zero_rows = sorted({0, n // 2, n - 1}) if n > 1 else []
    for r in zero_rows:
        X[r] = 0.0
    U = host(engine.rows_unit(dev(X)))
    ratio = worst_ratio(U, sr.unit(X), sr.unit_bound(k))
    report("rows_unit", f"n={n} k={k}", ratio)
    assert ratio <= 1.0
    for r in zero_rows:
        assert not U[r].any(), f"zero row {r} must give zeros exactly"
    assert np.isfinite(U).all()


def test_rows_unit_single_zero_row_and_floor(engine):
    """n = 1 with a zero row, and a row shorter than the floor 1e-12: divided by the floor (documented), not normalised."""
    assert not host(engine.rows_unit(dev(np.zeros((1, 32), dtype=np.float32)))).any()
    X = np.zeros((2, 3), dtype=np.float32)
    X[0] = [3e-20, 0, 4e-20]
    X[1] = [3, 0, 4]
    U = host(engine.rows_unit(dev(X)))
    want = sr.unit(X)
    assert np.abs(U[0] - want[0]).max() <= 4 * sr.U24 * np.abs(want[0]).max()      # two roundings, of 1 / floor and of the product
    assert np.abs(U[1] - want[1]).max() <= sr.unit_bound(3)


# ------------------------------------------------------------------ kmeans_mindist
@pytest.mark.parametrize("n,k", sr.NK_CASES)
def test_kmeans_mindist(engine, n, k):
    seed = sr.case_seed(n, k)
    Ri, ci = sr.int_rows(n, k, seed), sr.int_rows(1, k, seed + 3)[0]
    d2 = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    out = engine.kmeans_mindist(dev(Ri), dev(ci), d2, first=True)
    assert out is d2
    first64 = sr.mindist(Ri, ci, None, True)
    assert exact(host(d2), first64), "first = True must overwrite every element of a NaN-filled d2 with the exact distance"
    prev = np.random.default_rng(seed + 9).integers(0, int(first64.max()) + 2, size=n).astype(np.float32)
    d2 = dev(prev)
    engine.kmeans_mindist(dev(Ri), dev(ci), d2, first=False)
    assert exact(host(d2), sr.mindist(Ri, ci, prev, False))
    R, c = sr.real_rows(n, k, seed + 10), sr.real_rows(1, k, seed + 11)[0]
    full64 = sr.mindist(R, c, None, True)
    d2 = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    engine.kmeans_mindist(dev(R), dev(c), d2, first=True)
    worst = worst_ratio(host(d2), full64, sr.dist2_bound(k, full64))
    prev = np.random.default_rng(seed + 12).uniform(0, 2 * np.median(full64) + 1e-3, n).astype(np.float32)     # about half the rows keep prev
    d2 = dev(prev)
    engine.kmeans_mindist(dev(R), dev(c), d2, first=False)
    worst = max(worst, worst_ratio(host(d2), sr.mindist(R, c, prev, False), sr.dist2_bound(k, full64)))
    report("kmeans_mindist", f"n={n} k={k}", worst)
    assert worst <= 1.0


# ------------------------------------------------------------------ kmeans_assign
def check_sums(R, lab, ps, pc, kc):
    """Counts per block = the bincount of that block's device labels; sums = the exact fp32 chain for those labels, bit for bit."""
    n = R.shape[0]
    want_ps, want_pc = sr.block_sums_f32(R, lab, kc)
    valid = lab[lab >= 0]
    assert np.array_equal(pc.sum(0), np.bincount(valid, minlength=kc))
    for b in range((n + 255) // 256):
        blk = lab[b * 256:(b + 1) * 256]
        assert np.array_equal(pc[b], np.bincount(blk[blk >= 0], minlength=kc)), f"block {b}"
    assert np.array_equal(pc, want_pc)
    assert ps.shape == want_ps.shape and np.array_equal(sr.bits(ps), sr.bits(want_ps)), "part_sum differs from the fp32 chain in row order"


@pytest.mark.parametrize("n,k,kc", sr.NKC_CASES)
def test_kmeans_assign(engine, n, k, kc):
    Ri, Ci = sr.int_label_case(n, k, kc)
    lab, d2, ps, pc = (host(t) for t in engine.kmeans_assign(dev(Ri), dev(Ci)))
    lab64, d64, _ = sr.assign(Ri, Ci)
    assert exact(d2, d64)
    assert lab.dtype == np.int32 and np.array_equal(lab, lab64), "integer distances are exact: every label, ties included, is the reference's"
    check_sums(Ri, lab, ps, pc, kc)

    R, C = sr.label_case(n, k, kc)
    Rd, Cd = dev(R), dev(C)
    lab, d2, ps, pc = (host(t) for t in engine.kmeans_assign(Rd, Cd))
    lab64, d64, margin = sr.assign(R, C)
    keep = sr.decisive(k, d64, margin)
    ratio = worst_ratio(d2, d64, sr.dist2_bound(k, d64)) if (lab == lab64).all() else \
        worst_ratio(d2[lab == lab64], d64[lab == lab64], sr.dist2_bound(k, d64[lab == lab64]))
    fin = margin[np.isfinite(margin)]
    report("kmeans_assign dist2", f"n={n} k={k} kc={kc}", ratio,
           f", decisive rows {int(keep.sum())} / {n}, labels differing on the others {int((lab != lab64)[~keep].sum())}, smallest margin / (2 bound) = "
           f"{float((margin / (2 * sr.dist2_bound(k, d64) + 1e-300)).min()):.3g}" + (f", median margin {float(np.median(fin)):.3g}" if fin.size else ""))
    assert keep.mean() >= 0.95
    assert np.array_equal(lab[keep], lab64[keep])
    # a row whose label differs (only possible on a near-tie) still reports the distance to ITS centre: within the bound of the second best
    other = lab != lab64
    assert (np.abs(d2[other] - d64[other]) <= margin[other] + sr.dist2_bound(k, d64[other] + margin[other])).all()
    assert ratio <= 1.0
    check_sums(R, lab, ps, pc, kc)
    lab_b, d2_b, ps_b, pc_b = engine.kmeans_assign(Rd, Cd, want_sums=False)
    assert ps_b is None and pc_b is None
    assert np.array_equal(host(lab_b), lab) and np.array_equal(sr.bits(host(d2_b)), sr.bits(d2)), "want_sums must not change label or dist2"
    again = [host(t) for t in engine.kmeans_assign(Rd, Cd)]
    assert np.array_equal(again[0], lab) and np.array_equal(again[3], pc)
    assert np.array_equal(sr.bits(again[1]), sr.bits(d2)) and np.array_equal(sr.bits(again[2]), sr.bits(ps)), "two runs must be bit-identical"


@pytest.mark.parametrize("n,k", [(257, 32), (513, 1), (256, 7)])
def test_kmeans_assign_ties_go_to_the_lowest_centre(engine, n, k):
    """Centres 1 and 3 are identical, centre 0 and centre 2 differ by 2 in one coordinate, and the integer rows sit exactly between them
    or on the twin centres: every comparison is an exact tie in fp32 and in float64, and the lower index must win."""
    rng = np.random.default_rng(sr.case_seed(n, k) + 13)
    base = rng.integers(-3, 4, size=k).astype(np.float32)
    C = np.stack([base, base + 20, base, base + 20]).astype(np.float32)
    C[0, 0] -= 1                                      # centre 0 = base - e0, centre 2 = base + e0: rows at base are exactly between
    C[2, 0] += 1
    R = np.tile(base, (n, 1)).astype(np.float32)
    R[1::2] = base + 20                               # odd rows sit on the twin centres 1 == 3
    lab, d2, ps, pc = (host(t) for t in engine.kmeans_assign(dev(R), dev(C)))
    lab64, d64, margin = sr.assign(R, C)
    assert (margin == 0.0).all()
    assert np.array_equal(lab64[:2], [0, 1]) and np.array_equal(lab, lab64)
    assert set(lab.tolist()) <= {0, 1} and exact(d2, d64)
    check_sums(R, lab, ps, pc, 4)
    assert not pc[:, 2:].any() and not sr.bits(ps[:, 2:]).any()


def test_kmeans_assign_more_centres_than_rows_and_a_far_centre(engine):
    """kc > n (one row, 31 centres), and a centre far from every row: count 0 and sums +0.0 in every block."""
    R, C = sr.label_case(1, 7, 31)
    lab, d2, ps, pc = (host(t) for t in engine.kmeans_assign(dev(R), dev(C)))
    lab64, d64, margin = sr.assign(R, C)
    assert margin[0] > 2 * sr.dist2_bound(7, d64[0]) and lab[0] == lab64[0]
    assert abs(d2[0] - d64[0]) <= sr.dist2_bound(7, d64[0])
    assert pc.shape == (1, 31) and pc.sum() == 1 and pc[0, lab[0]] == 1
    check_sums(R, lab, ps, pc, 31)
    R, C = sr.label_case(513, 16, 2)
    C = np.concatenate([C[:1], np.full((1, 16), 1e4, dtype=np.float32), C[1:]])
    lab, d2, ps, pc = (host(t) for t in engine.kmeans_assign(dev(R), dev(C)))
    assert not (lab == 1).any() and not pc[:, 1].any()
    assert not sr.bits(ps[:, 1]).any(), "the sums of an empty cluster are +0.0"
    assert pc.sum() == 513
    check_sums(R, lab, ps, pc, 3)


def test_kmeans_assign_nan_row(engine):
    """A row holding a NaN compares below nothing: label -1, dist2 +inf, in no sum and no count (Engine.kmeans_assign's docstring).  The
    other rows of its block, and the other blocks, are as without it; row 256 is the only row of its block."""
    n, k, kc = 257, 7, 5
    R, C = sr.label_case(n, k, kc)
    clean = [host(t) for t in engine.kmeans_assign(dev(R), dev(C))]
    Rn = R.copy()
    bad = [100, 256]
    Rn[100, 3] = np.nan
    Rn[256] = np.nan
    lab, d2, ps, pc = (host(t) for t in engine.kmeans_assign(dev(Rn), dev(C)))
    assert lab[bad].tolist() == [-1, -1] and np.isposinf(d2[bad]).all()
    ok = np.ones(n, dtype=bool)
    ok[bad] = False
    assert np.array_equal(lab[ok], clean[0][ok]) and np.array_equal(sr.bits(d2[ok]), sr.bits(clean[1][ok]))
    assert pc.sum() == n - 2 and not pc[1].any() and not sr.bits(ps[1]).any()
    assert np.isfinite(ps).all()
    check_sums(Rn, lab, ps, pc, kc)
    lab_b, d2_b, _, _ = engine.kmeans_assign(dev(Rn), dev(C), want_sums=False)
    assert np.array_equal(host(lab_b), lab) and np.array_equal(sr.bits(host(d2_b)), sr.bits(d2))


def test_kmeans_with_a_nan_row_is_refused_by_name(engine):
    """cluster._kmeans hands the -1 label of a NaN row on; canonical_labels, which used to index remap[-1] with it (the row silently joined
    the last cluster), raises a ValueError naming the row."""
    R = sr.unit(sr.real_rows(300, 4, 5)).astype(np.float32)
    R[17, 2] = np.nan
    lab = host(CL._kmeans(engine, CL._Comm(None), dev(R), 0, 300, 4, 3))
    assert lab[17] == -1 and (np.delete(lab, 17) >= 0).all()
    with pytest.raises(ValueError, match=r"row 17 .*label -1"):
        CL.canonical_labels(lab)


# ------------------------------------------------------------------ chol_inverse
def _near_dependent_gram(k, seed):
    """Y^T Y in fp32 with the last column = the first + 5 % of an independent one: the last pivot is ~2.5e-3 of its diagonal entry."""
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((200, k))
    Y[:, k - 1] = Y[:, 0] + 0.05 * rng.standard_normal(200)
    G = (Y.T @ Y).astype(np.float32)
    G[0, k - 1] += np.float32(1e-3)                   # slightly asymmetric: symmetrised inside
    return G


@pytest.mark.parametrize("k", [2, 31])
@pytest.mark.parametrize("shift_ppb", [0, 10_000, 1_000_000])
def test_chol_inverse_shifted(engine, k, shift_ppb):
    """Rinv against the reference on (G + G^T) / 2 + s I, s = shift_ppb 1e-9 mean(diag G), to the 1e-6 relative tolerance of
    test_chol_inverse_on_device; the near-dependent last column makes the shift move Rinv by far more than that."""
    G = _near_dependent_gram(k, 40 + k)
    want, piv, diag = sr.chol_inverse(G, shift_ppb * 1e-9)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    engine.set_option("chol_shift_ppb", shift_ppb)
    try:
        Rinv = host(engine.chol_inverse(dev(G), flag)).astype(np.float64)
    finally:
        engine.set_option("chol_shift_ppb", 0)
    rel = float(np.abs(Rinv - want).max() / np.abs(want).max())
    moved = float(np.abs(sr.chol_inverse(G, 0.0)[0] - want).max() / np.abs(want).max())
    report("chol_inverse", f"k={k} shift_ppb={shift_ppb}", rel / 1e-6, f" (the shift moves Rinv by {moved:.2e} relative; last pivot / diagonal {piv[-1] / diag[-1]:.3e})")
    assert rel <= 1e-6
    assert shift_ppb == 0 or moved > 100e-6
    assert not np.tril(Rinv, -1).any() and int(flag.item()) == 0
    plain = host(engine.chol_inverse(dev(G))).astype(np.float64)                       # the option is restored: unshifted again
    assert np.abs(plain - sr.chol_inverse(G, 0.0)[0]).max() <= 1e-6 * np.abs(plain).max()


def test_chol_inverse_default_pivot_rule(engine):
    """The default rule flags a pivot <= 1e-6 of its diagonal entry.  G = [[1, c], [c, 1]] has the last pivot 1 - c^2 exactly (float64):
    c = 1 - 9 * 2^-24 gives 1.073e-6 (not flagged), c = 1 - 8 * 2^-24 gives 9.54e-7 (flagged)."""
    for m, want_flag in ((9, 0), (8, 1)):
        c = np.float32(1.0 - m * 2.0 ** -24)
        G = np.array([[1, c], [c, 1]], dtype=np.float32)
        _, piv, diag = sr.chol_inverse(G)
        assert (piv[1] / diag[1] > 1e-6) == (want_flag == 0)
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        engine.chol_inverse(dev(G), flag)
        assert int(flag.item()) == want_flag, (m, piv[1])


@pytest.mark.parametrize("k,shift_ppb", [(2, 0), (31, 0), (31, 10_000)])
def test_chol_inverse_relative_pivot_option(engine, k, shift_ppb):
    """chol_pivot_rtol_ppb two parts in 1e9 below the last pivot's share of its (shifted) diagonal entry: not flagged; two above: flagged."""
    G = _near_dependent_gram(k, 60 + k)
    _, piv, diag = sr.chol_inverse(G, shift_ppb * 1e-9)
    ratios = piv / diag * 1e9
    last = float(ratios[-1])
    assert 1e5 < last < 1e8 and (k == 2 or ratios[:-1].min() > 10 * last)               # only the last pivot is near the rule
    try:
        engine.set_option("chol_shift_ppb", shift_ppb)
        for rtol, want_flag in ((int(np.floor(last)) - 2, 0), (int(np.ceil(last)) + 2, 1)):
            engine.set_option("chol_pivot_rtol_ppb", rtol)
            flag = torch.zeros(1, dtype=torch.int32, device="cuda")
            engine.chol_inverse(dev(G), flag)
            assert int(flag.item()) == want_flag, (rtol, last)
    finally:
        engine.set_option("chol_pivot_rtol_ppb", 1000)
        engine.set_option("chol_shift_ppb", 0)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    engine.chol_inverse(dev(G), flag)
    assert int(flag.item()) == 0                                                         # the default rule (1e-6) is back


# ------------------------------------------------------------------ affinity_matvec, small shapes and paths
def _unit_rows(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _matvec_case(engine, N, kv, row0, rows, use_xscale, use_out):
    """The rule of test_gpu_kernels._check_matvec: within 1.5e-3 of the row's absolute sum.  The kernel rounds S = max(E E^T, 0) to bf16
    (up to 2^-9 = 1.95e-3 relative per term), and the rule counts on the terms of a row averaging out.  At N <= 32 they are too few for
    that: with gaussian X an element whose own x_i is small is carried by a handful of off-diagonal terms, and the rounding of S alone
    reaches 1.16 of the rule (N = 32, kv = 16, simulated on the host).  So the small cases keep |x| and xscale in [0.75, 1.25]: every
    element then holds its diagonal term S_ii |x_i| ~ 1 (S_ii is within 1e-3 of 1 and rounds to 1.0) beside off-diagonal terms that sum
    to <= 1.4 here, i.e. at most (1e-3 * 0.56 + 1.95e-3 * 1.4 * 1.56) / (0.56 + 1.4 * 1.56) = 1.75e-3 in the worst alignment of every
    rounding and well under 1.5e-3 otherwise (simulated: <= 0.73 of the rule)."""
    _, Eb, _ = engine.l2norm(dev(_unit_rows(N, 192, 900 + N)))
    Ef = host(Eb.float()).astype(np.float64)                                             # the kernel sees the bf16 rows
    rng = np.random.default_rng(sr.case_seed(N, kv))
    if N > 32:
        X = rng.standard_normal((N, kv)).astype(np.float32)
        xs = rng.uniform(0.5, 1.5, N).astype(np.float32) if use_xscale else None
    else:
        X = (rng.uniform(0.75, 1.25, (N, kv)) * rng.choice([-1.0, 1.0], (N, kv))).astype(np.float32)
        xs = rng.uniform(0.75, 1.25, N).astype(np.float32) if use_xscale else None
    before = rng.uniform(1.0, 2.0, (N, kv)).astype(np.float32)                          # non-zero everywhere
    out = dev(before) if use_out else None
    Y = engine.affinity_matvec(Eb, dev(X), row0, rows, xscale=None if xs is None else dev(xs), out=out)
    assert out is None or Y is out
    got = host(Y)
    A = np.maximum(Ef[row0:row0 + rows] @ Ef.T, 0.0)
    Xs = X.astype(np.float64) * (1.0 if xs is None else xs.astype(np.float64)[:, None])
    want = A @ Xs
    scale = A @ np.abs(Xs) + 1e-6
    ratio = float((np.abs(got[row0:row0 + rows] - want) / (1.5e-3 * scale)).max())
    report("affinity_matvec", f"N={N} kv={kv} rows=[{row0}, {row0 + rows}) xscale={'yes' if use_xscale else 'None'} out={'yes' if use_out else 'no'}", ratio)
    assert ratio <= 1.0
    outside = np.ones(N, dtype=bool)
    outside[row0:row0 + rows] = False
    if use_out:
        assert np.array_equal(sr.bits(got[outside]), sr.bits(before[outside])), "rows outside the block must keep their contents"
    else:
        assert not got[outside].any()


@pytest.mark.parametrize("N,kv", [(1, 1), (1, 32), (31, 7), (32, 16), (32, 32)])
@pytest.mark.parametrize("use_xscale", [True, False])
def test_affinity_matvec_small(engine, N, kv, use_xscale):
    _matvec_case(engine, N, kv, 0, N, use_xscale, False)


@pytest.mark.parametrize("N,kv,row0,rows", [(700, 5, 200, 300), (32, 32, 9, 14), (31, 2, 30, 1)])
def test_affinity_matvec_out_keeps_the_rows_outside_the_block(engine, N, kv, row0, rows):
    _matvec_case(engine, N, kv, row0, rows, True, True)
    _matvec_case(engine, N, kv, row0, rows, False, True)


# ------------------------------------------------------------------ the wrappers refuse what the kernels would misread
def test_thin_wrappers_refuse_bad_arguments(engine):
    """A float64 block, a column slice, a Y shaped differently from X, centres of another width, k or kc outside 1..32: ValueError naming
    the argument, before any launch - and the next valid call still works."""
    n, k, kc = 40, 8, 3
    X = dev(sr.real_rows(n, k, 1))
    Y = dev(sr.real_rows(n, k, 2))
    R = dev(sr.real_rows(k, k, 3))
    C = dev(sr.real_rows(kc, k, 4))
    sc = dev(sr.pow2_scale(n, 5))
    wide = dev(sr.real_rows(n, 2 * k, 6))
    d2 = torch.zeros(n, dtype=torch.float32, device="cuda")
    X33, C33 = dev(sr.real_rows(n, 33, 7)), dev(sr.real_rows(33, k, 8))
    empty = torch.zeros((n, 0), dtype=torch.float32, device="cuda")
    valid = {
        "rows_gram": lambda: engine.rows_gram(X, Y),
        "rows_apply": lambda: engine.rows_apply(X, R, sc),
        "rows_unit": lambda: engine.rows_unit(X),
        "kmeans_mindist": lambda: engine.kmeans_mindist(X, C[0], d2, True),
        "kmeans_assign": lambda: engine.kmeans_assign(X, C),
    }
    want = {name: [host(t).copy() for t in (r if isinstance(r, tuple) else (r,))] for name, r in ((nm, f()) for nm, f in valid.items())}
    refusals = [
        ("rows_gram", "X", lambda: engine.rows_gram(X.double(), Y)),
        ("rows_gram", "X", lambda: engine.rows_gram(wide[:, :k], Y)),
        ("rows_gram", "Y", lambda: engine.rows_gram(X, Y.double())),
        ("rows_gram", "Y", lambda: engine.rows_gram(X, wide[:, :k])),
        ("rows_gram", "Y", lambda: engine.rows_gram(X, Y[:-1])),
        ("rows_gram", "Y", lambda: engine.rows_gram(X, wide)),
        ("rows_gram", "k", lambda: engine.rows_gram(X33, X33)),
        ("rows_gram", "k", lambda: engine.rows_gram(empty, empty)),
        ("rows_gram", "X", lambda: engine.rows_gram(X.cpu(), Y)),
        ("rows_apply", "X", lambda: engine.rows_apply(X.half(), R)),
        ("rows_apply", "X", lambda: engine.rows_apply(wide[:, ::2], R)),
        ("rows_apply", "R", lambda: engine.rows_apply(X, R.double())),
        ("rows_apply", "R", lambda: engine.rows_apply(X, R[:, :-1])),
        ("rows_apply", "scale", lambda: engine.rows_apply(X, R, sc.double())),
        ("rows_apply", "scale", lambda: engine.rows_apply(X, R, sc[:-1])),
        ("rows_apply", "k", lambda: engine.rows_apply(X33, dev(np.eye(33, dtype=np.float32)))),
        ("rows_unit", "X", lambda: engine.rows_unit(X.double())),
        ("rows_unit", "X", lambda: engine.rows_unit(X.t())),
        ("rows_unit", "k", lambda: engine.rows_unit(X33)),
        ("kmeans_mindist", "R", lambda: engine.kmeans_mindist(X.double(), C[0], d2, True)),
        ("kmeans_mindist", "R", lambda: engine.kmeans_mindist(wide[:, :k], C[0], d2, True)),
        ("kmeans_mindist", "centre", lambda: engine.kmeans_mindist(X, C[0, :-1], d2, True)),
        ("kmeans_mindist", "centre", lambda: engine.kmeans_mindist(X, C[0].double(), d2, True)),
        ("kmeans_mindist", "d2", lambda: engine.kmeans_mindist(X, C[0], d2.double(), True)),
        ("kmeans_mindist", "d2", lambda: engine.kmeans_mindist(X, C[0], torch.zeros(2 * n, device="cuda")[::2], True)),
        ("kmeans_mindist", "d2", lambda: engine.kmeans_mindist(X, C[0], d2[:-1], True)),
        ("kmeans_assign", "R", lambda: engine.kmeans_assign(X.double(), C)),
        ("kmeans_assign", "R", lambda: engine.kmeans_assign(wide[:, :k], C)),
        ("kmeans_assign", "centres", lambda: engine.kmeans_assign(X, C.double())),
        ("kmeans_assign", "centres", lambda: engine.kmeans_assign(X, C[:, :-1])),
        ("kmeans_assign", "centres", lambda: engine.kmeans_assign(X, C[0])),
        ("kmeans_assign", "kc", lambda: engine.kmeans_assign(X, C33)),
        ("kmeans_assign", "kc", lambda: engine.kmeans_assign(X, C[:0])),
        ("kmeans_assign", "k", lambda: engine.kmeans_assign(X33, dev(sr.real_rows(2, 33, 9)))),
    ]
    for name, arg, call in refusals:
        with pytest.raises(ValueError, match=rf"{name}: .*\b{arg}\b"):
            call()
        r = valid[name]()
        r = r if isinstance(r, tuple) else (r,)
        for got, w in zip(r, want[name]):
            assert np.array_equal(host(got), w), f"{name}: the valid call after a refusal ({arg}) differs"
    # a centres view that .contiguous() covers is still taken
    lab = host(engine.kmeans_assign(X, dev(sr.real_rows(kc, 2 * k, 4))[:, :k])[0])
    assert lab.shape == (n,) and (lab >= 0).all()
