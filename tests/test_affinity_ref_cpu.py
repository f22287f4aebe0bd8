"""The host restatement of the affinity exact pass (tests/affinity_ref.py) on its own: its fma against rational arithmetic, its scores against
the float64 scan, its tie rule, and every fixture condition the GPU test relies on - so that a wrong restatement or a bad fixture fails here,
without a GPU."""
from fractions import Fraction

import numpy as np
import pytest

import affinity_ref as R


def _round_f32(x: Fraction) -> np.float32:
    """x correctly rounded (nearest, ties to even) to fp32: the nearest of a first guess and its two fp32 neighbours, by exact distance."""
    g = np.float32(float(x))
    cands = [np.nextafter(g, np.float32(-np.inf)), g, np.nextafter(g, np.float32(np.inf))]
    best = min(cands, key=lambda c: (abs(Fraction(float(c)) - x), int(np.float32(c).view(np.uint32)) & 1))
    return np.float32(best)


def _triples(n, seed):
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-12, 12, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-12, 12, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-24, 24, n)).astype(np.float32)
    q = n // 4                                                    # a quarter cancels almost completely: c ~ -a b
    c[:q] = (-(a[:q].astype(np.float64) * b[:q]) * (1 + rng.integers(-3, 4, q) * 2.0 ** -23)).astype(np.float32)
    c[q:2 * q] = (rng.standard_normal(q) * np.abs(a[q:2 * q] * b[q:2 * q])).astype(np.float32)      # a quarter with a comparable addend (the dot product's case)
    return a, b, c


def test_fma32_is_correctly_rounded():
    a, b, c = _triples(24000, 11)
    got = R.fma32(a, b, c)
    for i in range(a.size):
        want = _round_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert got[i].view(np.uint32) == want.view(np.uint32), (i, a[i], b[i], c[i], got[i], want)


def test_fma32_where_rounding_twice_goes_wrong():
    """a b = 1 + 2^-j + 2^-(24-j) + 2^-24 is an fp32 rounding MIDPOINT; an addend of +-2^-70 decides the direction but vanishes in float64, so the
    float64-rounded-once emulation rounds the tie to even - wrong for one of the two signs.  fma32 must follow the rational result on all of them,
    and the naive emulation must differ on at least one: the test can tell the two apart."""
    naive_wrong = 0
    for j in range(2, 12):
        a, b = np.float32(1 + 2.0 ** -j), np.float32(1 + 2.0 ** -(24 - j))
        for c in (np.float32(2.0 ** -70), np.float32(-2.0 ** -70), np.float32(2.0 ** -40), np.float32(-2.0 ** -40)):
            for sa in (1, -1):
                aa, cc = np.float32(sa * a), np.float32(sa * c)
                want = _round_f32(Fraction(float(aa)) * Fraction(float(b)) + Fraction(float(cc)))
                got = R.fma32(aa, b, cc)
                assert got.view(np.uint32) == want.view(np.uint32), (j, aa, b, cc, got, want)
                naive_wrong += int(R.fma32_naive(aa, b, cc).view(np.uint32) != want.view(np.uint32))
    assert naive_wrong >= 1, "no case separates the correctly rounded fma from the float64-rounded-once emulation"
    print(f"double-rounding cases on which the float64-rounded-once emulation is wrong: {naive_wrong} of 80")


SMALL = [("gauss", 33, 65), ("knots", 33, 65), ("knots", 5, 1025), ("dups", 4, 2049), ("ends", 9, 33), ("negative", 31, 63), ("zeros", 5, 64),
         ("zeros", 1, 31), ("gauss", 3, 4)]


def test_dot192_is_within_the_derived_bound_of_float64():
    """The bound.  A lane's sum is 24 sequential fma from 0: s_i = (s_{i-1} + e_i p_i)(1 + d_i), |d_i| <= u = 2^-24, so the product e_i p_i carries
    at most the factors (1 + d_i) .. (1 + d_24): 24 of them.  The butterfly adds three more levels, each one (1 + d): every product carries at
    most 27 factors, and |computed - exact| <= gamma_27 sum |e_i p_i| <= gamma_27 |e| |p| (Cauchy-Schwarz), gamma_n = n u / (1 - n u) (Higham,
    Accuracy and Stability of Numerical Algorithms, Lemma 3.1).  The float64 scan's own error, gamma64_192 |e| |p| < 3e-14 |e| |p|, is covered by
    1e-12.  With |e|, |p| the rows' norms (1 to within fp32 rounding; smaller for zero rows): bound = 1.61e-6 |e| |p| + 1e-12."""
    worst = 0.0
    for kind, N, P in SMALL:
        E, Pm, _ = R.KINDS[kind](N, P, 0)
        En, Pn = R.l2n(E), R.l2n(Pm)
        d = np.abs(R.dot192(En, Pn).astype(np.float64) - R.scan64(En, Pn))
        ne = np.sqrt((En.astype(np.float64) ** 2).sum(1))[:, None]
        npn = np.sqrt((Pn.astype(np.float64) ** 2).sum(1))[None]
        bound = R.GAMMA27 * ne * npn + 1e-12
        assert (d <= bound).all(), (kind, N, P, float(d.max()))
        worst = max(worst, float(d.max()))
    print(f"dot192 vs the float64 scan over the fixtures: max |d| = {worst:.3e}; bound gamma_27 |e| |p| + 1e-12 = {R.GAMMA27 + 1e-12:.3e} on unit rows")
    assert worst > 0, "the restatement equals float64: it is not an fp32 computation"


def test_the_pruned_topk_equals_the_full_scan():
    for kind, N, P in SMALL:
        E, Pm, _ = R.KINDS[kind](N, P, 1)
        En, Pn = R.l2n(E), R.l2n(Pm)
        for k in sorted({1, min(2, P), min(4, P)}):
            i0, s0 = R.topk(En, Pn, k, full=True)
            i1, s1 = R.topk(En, Pn, k)
            assert np.array_equal(i0, i1) and np.array_equal(s0.view(np.uint32), s1.view(np.uint32)), (kind, N, P, k)


def test_tie_rule_and_k_equal_p():
    S = np.array([[0.5, 0.7, 0.7, 0.1], [0.0, -0.0, 0.0, -1.0], [np.nan, 0.2, np.nan, 0.2]], dtype=np.float32)
    idx, sc = R.topk_of_scores(S, 4)
    assert idx.tolist() == [[1, 2, 0, 3], [0, 1, 2, 3], [1, 3, -1, -1]]          # higher score first, then the lower index; +0 == -0; NaN never taken
    assert sc[2].tolist()[:2] == [np.float32(0.2)] * 2 and np.isneginf(sc[2, 2:]).all()
    assert R.better(1.0, 5, 0.5, 0) and R.better(1.0, 2, 1.0, 3) and not R.better(1.0, 3, 1.0, 2) and not R.better(float("nan"), 0, -np.inf, 9)
    for P in (1, 2, 3, 4):                                                       # k == P: every profile, in order
        E, Pm, _ = R.gauss(3, P, 5)
        idx, sc = R.topk(E, Pm, P)
        full = R.dot192(E, Pm)
        for n in range(3):
            assert sorted(idx[n].tolist()) == list(range(P))
            assert all(R.better(sc[n, q], idx[n, q], sc[n, q + 1], idx[n, q + 1]) for q in range(P - 1))
            assert np.array_equal(full[n, idx[n]].view(np.uint32), sc[n].view(np.uint32))
    # a NaN segment row: every slot (-1, -inf); a NaN profile row: never taken
    E, Pm, _ = R.gauss(3, 5, 6)
    E[1, 7] = np.nan
    Pm[2, 100] = np.nan
    idx, sc = R.topk(E, Pm, 4)
    assert (idx[1] == -1).all() and np.isneginf(sc[1]).all() and not (idx == 2).any() and sorted(idx[0].tolist()) == [0, 1, 3, 4]
    idx, sc = R.topk(E, Pm, 5)
    assert idx[0, 4] == -1 and np.isneginf(sc[0, 4])


def _grid():
    import test_affinity_edges_gpu as G
    return sorted({(kind, N, P, seed) for kind, N, P, seed in G.FIXTURES})


def test_every_gpu_fixture_meets_its_condition_on_the_restatement():
    """The GPU test's fixtures (its own list), normalised on the host, scored by the restatement: the planted rows, duplicate pairs, end
    winners, signs and zero rows must come out as the fixture says, for every k the GPU test uses."""
    for kind, N, P, seed in _grid():
        E, Pm, info = R.KINDS[kind](N, P, seed)
        En, Pn = R.l2n(E), R.l2n(Pm)
        idx, sc = R.topk(En, Pn, min(4, P))                    # the k best are a prefix of these (a total order)
        for k in sorted({1, min(2, P), min(4, P)}):
            R.check_fixture(kind, info, En, Pn, idx[:, :k], sc[:, :k], k)
        if kind == "knots" and P > 32768:
            assert any((ko >= 32768).any() for ko in info["knot_of"]), "no knot reaches the last rescan slice"
