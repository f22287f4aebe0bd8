"""GPU checks of the PLDA log-likelihood-ratio scoring (sdk_plda_enroll, sdk_plda_score_topk; Engine.plda_enroll, Engine.plda_score_topk; the
Backend's PLDA identify path) against the independent float64 reference tests/plda_score_ref.py.

The score bound.  The score tests feed the kernel the REFERENCE's table (G, r), so only the kernel's own arithmetic separates the two sides.
An element is r_s + sum over 2 D products z_j G_sj, z = [x, x^2].  In the kernel a term meets at most: the rounding of x * x (the second half
only), the rounding of its product (none where the MFMA fuses it), the additions of its chain - 2 D of them, the first onto a zero
accumulator, which is exact, so 2 D - 1 - and the epilogue's addition of r_s: 2 D + 2 roundings, whatever the order of the chain.  With
u = 2^-53 that is gamma_(2 D + 2) A <= (2 D + 3) u A, A(n, s) = |r_s| + sum_d (|x_d G_sd| + |x_d^2 G_s,D+d|).  The reference
(plda_score_ref.llr_table) is the correctly rounded exact sum: u |llr| <= u A more.  So |device - reference| <= C u A with C = 2 D + 4.

The enrolment bound, per table entry (enrol_bounds): both sides pool a speaker's m rows in the same ascending order and then evaluate the
coefficients in float64, so each side's own rounding is counted once and the sum of both is the bound.
  u_s (the mean)   : |du| <= m u mean_p |x_pd|  (m - 1 additions and the division)
  g u              : den = n Phi + 1 (2 roundings), a = n Phi / den (4 u relative), v = 1 + Phi / den (4 u), a / v (9 u), times u_s (10 u):
                     |d(g u)| <= g |du| + 10 u |g u|
  q                : 1 / v (5 u, and 1 / v <= 1), 1 / (1 + Phi) (2 u, <= 1), their difference (u |difference| <= u), halved exactly: 4 u absolute
  r                : per column c_d = -(ln v - ln(1 + Phi)) / 2 with a logarithm good to 2 u relative and arguments off by 4 u and u:
                     (4 + 2 ln(1 + Phi)) u absolute, generously; h = -a^2 / (2 v) is good to 14 u relative, u_s^2 h to 16 u relative plus
                     2 |u_s h| |du|; the D column terms t_d are then added by a tree - at most 7 additions on the device (two columns per
                     lane, six shuffle levels), at most 19 in numpy's pairwise sum of 128 - 26 u sum_d |t_d| for both sides together.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plda_score_ref as PR  # noqa: E402
from conftest import ROOT, sub  # noqa: E402

pytestmark = pytest.mark.gpu

LIB = sub("_lib")
PLDA = sub("plda")
U53 = 2.0 ** -53
TILE, SPLIT = 64, 256            # csrc/plda_score.hip: speakers per tile; speakers per split (at least; four tiles)
_PHI = {}


def spectrum(D):
    if D not in _PHI:
        _PHI[D] = PLDA.synthetic_plda(192, 128, lda_dim=D).Phi
    return _PHI[D]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def score_bound(X, G, r):
    D = X.shape[1]
    return (2 * D + 4) * U53 * PR.magnitude(X, G, r)


def gpu_topk(engine, X, G, r, k, scores=True):
    out = engine.plda_score_topk(dev(X), dev(G), dev(r), k=k, scores=scores)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


_CASES = {}


def case(N, S, k, D):
    """Planted inputs, the reference table and the reference scores of a case, computed once."""
    key = (N, S, k, D)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * N + 10 * S + k + D)
        Phi = spectrum(D)
        X, Xp, group, counts = PR.planted(rng, N, S, D, Phi)
        G, r, _, _ = PR.table(Xp, group, counts.astype(np.float64), Phi)
        _CASES[key] = dict(X=X, Xp=Xp, group=group, counts=counts, G=G, r=r, L=PR.llr_table(X, G, r), B=score_bound(X, G, r))
    return _CASES[key]


def clear_rows(L, B, k):
    """Rows whose top-k the arithmetic cannot disturb: every gap down to rank k + 1 exceeds twice the larger neighbour's bound."""
    N, S = L.shape
    order = np.argsort(-L, axis=1, kind="stable")
    Ls, Bs = np.take_along_axis(L, order, 1), np.take_along_axis(B, order, 1)
    kk = min(k, S - 1)
    if kk == 0:
        return np.ones(N, bool)
    gaps = Ls[:, :kk] - Ls[:, 1:kk + 1]
    return (gaps > 2 * np.maximum(Bs[:, :kk], Bs[:, 1:kk + 1])).all(axis=1)


# S = 2085 crosses eight full splits of 256 speakers and a partial one (32 full tiles of 64 and a partial one); (130, 300) adds three
# window tiles, the last one partial, against two splits
SCORE_CASES = [(1, 1, 1, 64), (33, 1, 1, 128), (70, 100, 1, 128), (70, 100, 4, 64), (70, 3, 3, 128), (5, 2085, 4, 128), (130, 300, 4, 128)]
_worst = {}


@pytest.mark.parametrize("N,S,k,D", SCORE_CASES)
def test_score_topk_against_float64(engine, N, S, k, D):
    c = case(N, S, k, D)
    L, B = c["L"], c["B"]
    ok = clear_rows(L, B, k)
    assert (~ok).sum() <= 0.01 * N, f"{int((~ok).sum())} of {N} rows excused by the reference alone"
    ridx, rsc = PR.topk(L, min(k, S))
    idx, sc, full = gpu_topk(engine, c["X"], c["G"], c["r"], k)
    assert idx.shape == (N, k) and idx.dtype == np.int32 and sc.shape == (N, k) and sc.dtype == np.float64 and full.shape == (N, S)
    kw = min(k, S)
    idx, sc = idx[:, :kw], sc[:, :kw]
    n = np.arange(N)[:, None]
    ratio_full = float((np.abs(full - L) / B).max())
    assert (idx >= 0).all() and (idx < S).all()
    ratio_sc = float((np.abs(sc - L[n, idx]) / B[n, idx]).max())
    _worst[(N, S, k, D)] = max(ratio_full, ratio_sc)
    print(f"plda_score_topk N={N} S={S} k={k} D={D}: {int((~ok).sum())} rows excused, worst |scores - ref| / bound = {ratio_full:.4f}, "
          f"worst |score - ref| / bound = {ratio_sc:.4f}, worst bound {float(B.max()):.3e} (so far over all cases: {max(_worst.values()):.4f})")
    assert np.array_equal(idx[ok], ridx[ok])
    assert (np.abs(sc - L[n, idx]) <= B[n, idx]).all()
    assert (np.abs(full - L) <= B).all()
    assert np.array_equal(sc, full[n, idx])                                # bit for bit
    idx2, sc2 = gpu_topk(engine, c["X"], c["G"], c["r"], k, scores=False)  # two runs; with and without the full matrix
    assert np.array_equal(idx2[:, :kw], idx) and np.array_equal(sc2[:, :kw], sc)


def test_columns_beyond_the_speakers_are_not_written(engine):
    c = case(70, 3, 3, 128)
    idx = torch.full((70, 4), 77, dtype=torch.int32, device="cuda")
    sc = torch.full((70, 4), 7.5, dtype=torch.float64, device="cuda")
    X, G, r = dev(c["X"]), dev(c["G"]), dev(c["r"])
    lib = LIB.load_library()
    ws = torch.empty(lib.sdk_plda_score_workspace_bytes(70, 3, 4), dtype=torch.uint8, device="cuda")
    rc = lib.sdk_plda_score_topk(engine.ctx, X.data_ptr(), 70, 128, G.data_ptr(), r.data_ptr(), 3, 4, idx.data_ptr(), sc.data_ptr(), None,
                                 ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert (idx[:, 3] == 77).all() and (sc[:, 3] == 7.5).all() and (idx[:, :3] >= 0).all() and (idx[:, :3] < 3).all()


# ---- enrolment --------------------------------------------------------------------------------------------------------------------------
def enrol_bounds(Xp, group, n_eff, Phi):
    """(bound on G [S, 2 D], bound on r [S]) per the module docstring, from the reference's own quantities."""
    S, D = len(n_eff), len(Phi)
    _, _, Uref, m = PR.table(Xp, group, n_eff, Phi)
    ok = PR.valid(m, n_eff)
    meanabs = np.zeros((S, D))
    for p in range(len(group)):
        if 0 <= group[p] < S:
            meanabs[group[p]] += np.abs(Xp[p])
    meanabs /= np.maximum(m, 1)[:, None]
    bG, br = np.zeros((S, 2 * D)), np.zeros(S)
    for s in np.flatnonzero(ok):
        n = float(n_eff[s])
        a = n * Phi / (n * Phi + 1)
        v = 1 + Phi / (n * Phi + 1)
        g, h = a / v, a * a / (2 * v)
        du = m[s] * U53 * meanabs[s]
        u = np.abs(Uref[s])
        bG[s, :D] = 2 * (g * du + 10 * U53 * g * u)
        bG[s, D:] = 2 * 4 * U53
        t = np.abs(0.5 * (np.log(v) - np.log(1 + Phi))) + u * u * h
        br[s] = (2 * ((4 + 2 * np.log(1 + Phi)) * U53 + 16 * U53 * u * u * h + 2 * u * h * du)).sum() + 26 * U53 * t.sum()
    return bG, br


def carried_bound(Xw, G, r, Xp, group, n_eff, Phi):
    """The bound on a device score whose TABLE is the device's own: the scoring arithmetic (A is formed from the reference's table; the
    device's differs from it by bG, a relative 1e-13 of A at most - the factor 1.01 covers it) plus the table's bounds carried through
    the score, |x| bG + x^2 bq + br."""
    bG, br = enrol_bounds(Xp, group, n_eff, Phi)
    D = Xw.shape[1]
    return score_bound(Xw, G, r) * 1.01 + np.abs(Xw) @ bG[:, :D].T + (Xw * Xw) @ bG[:, D:].T + br[None, :]


def gpu_enroll(engine, Xp, group, n_eff, Phi):
    G, r, status = engine.plda_enroll(dev(Xp), dev(group), dev(n_eff), dev(Phi))
    torch.cuda.synchronize()
    return G.cpu().numpy(), r.cpu().numpy(), int(status.item())


@pytest.mark.parametrize("D", [64, 128])
def test_enroll_against_float64(engine, D):
    rng = np.random.default_rng(D + 5)
    Phi = spectrum(D)
    S = 300                                                              # more than one block of four speakers; speakers of 1 .. 5 rows ..
    _, Xp, group, counts = PR.planted(rng, 1, S, D, Phi)
    extra = rng.standard_normal((40, D)) + 1.0                           # .. speaker 7 gets 40 rows more, scattered; speaker 9 exactly one
    keep = group != 9
    Xp, group = Xp[keep], group[keep]
    Xp = np.concatenate([Xp, extra, rng.standard_normal((1, D))])
    group = np.concatenate([group, np.full(40, 7, np.int32), np.asarray([9], np.int32)])
    perm = rng.permutation(len(group))
    Xp, group = np.ascontiguousarray(Xp[perm]), np.ascontiguousarray(group[perm])          # interleaved and unsorted
    none = group != 11
    Xp, group = np.ascontiguousarray(Xp[none]), np.ascontiguousarray(group[none])          # speaker 11 has no row
    n_eff = np.bincount(group, minlength=S).astype(np.float64)
    n_eff[11] = 1.0
    n_eff[12], n_eff[13], n_eff[14] = 0.0, np.nan, 2.5                   # 0 and NaN: never win; a non-integer count
    n_eff[15] = np.inf
    G, r, status = gpu_enroll(engine, Xp, group, n_eff, Phi)
    Gr, rr, _, m = PR.table(Xp, group, n_eff, Phi)
    assert m[7] >= 41 and m[9] == 1 and m[11] == 0 and status == 0
    bad = [11, 12, 13, 15]
    assert np.isnan(r[bad]).all() and not G[bad].any() and np.isnan(rr[bad]).all()
    good = np.setdiff1d(np.arange(S), bad)
    bG, br = enrol_bounds(Xp, group, n_eff, Phi)
    eg, er = np.abs(G - Gr)[good], np.abs(r - rr)[good]
    print(f"plda_enroll D={D}: worst |G - ref| / bound = {float((eg / bG[good]).max()):.4f}, worst |r - ref| / bound = {float((er / br[good]).max()):.4f}")
    assert (eg <= bG[good]).all() and (er <= br[good]).all()
    G2, r2, _ = gpu_enroll(engine, Xp, group, n_eff, Phi)
    assert np.array_equal(G, G2) and np.array_equal(r, r2, equal_nan=True)
    # an out-of-range label: the status bit, and every entry of the in-range speakers as without it
    Xo = np.concatenate([Xp[:5], rng.standard_normal((2, D)), Xp[5:]])
    go = np.concatenate([group[:5], np.asarray([S, -3], np.int32), group[5:]])
    G3, r3, status3 = gpu_enroll(engine, np.ascontiguousarray(Xo), np.ascontiguousarray(go), n_eff, Phi)
    assert status3 & 1 and np.array_equal(G3, G) and np.array_equal(r3, r, equal_nan=True)
    # the NaN speakers never win; their duplicates (same rows, a valid count) do
    X = rng.standard_normal((6, D))
    idx, sc = gpu_topk(engine, X, G, r, 4, scores=False)
    assert not np.isin(idx, bad).any() and (idx >= 0).all()


# ---- ties, NaN ----------------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_speaker_and_a_nan_never_wins(engine):
    D = 128
    c = case(5, 2085, 4, 128)
    rng = np.random.default_rng(77)
    S = 700                                                              # three splits of 256 speakers
    G, r = c["G"][:S].copy(), c["r"][:S].copy()
    X = rng.standard_normal((9, D)) * np.sqrt(1 + spectrum(D))
    hot = 3.0 * G[5, :D] / np.abs(G[5, :D]).max()                        # windows near speaker 5's direction: its copies lead the row
    X[:4] = hot + 0.1 * rng.standard_normal((4, D))
    for dup in (6, 5 + TILE, 5 + SPLIT + 70, S - 1):                     # the same tile, another tile of the split, other splits
        G[dup], r[dup] = G[5], r[5]
    L = PR.llr_table(X, G, r)
    assert (np.argmax(L[:4], axis=1) == 5).all()
    idx, sc, full = gpu_topk(engine, X, G, r, 4)
    assert idx[:4].tolist() == [[5, 6, 5 + TILE, 5 + SPLIT + 70]] * 4
    assert (sc[:4] == sc[:4, :1]).all() and (full[:4, S - 1] == sc[:4, 0]).all()
    ridx, _ = PR.topk(L, 4)
    ok = clear_rows(np.delete(L, [6, 5 + TILE, 5 + SPLIT + 70, S - 1], axis=1), np.delete(score_bound(X, G, r), [6, 5 + TILE, 5 + SPLIT + 70, S - 1], axis=1), 4)
    assert np.array_equal(idx[4:][ok[4:]], ridx[4:][ok[4:]])
    # a NaN speaker is skipped and its duplicate takes the slot
    r2 = r.copy()
    r2[5] = np.nan
    idx2, sc2 = gpu_topk(engine, X, G, r2, 4, scores=False)
    assert idx2[:4].tolist() == [[6, 5 + TILE, 5 + SPLIT + 70, S - 1]] * 4 and np.array_equal(sc2[:4, 0], sc[:4, 0])
    # a NaN in a window: -1 and 0 in all k slots, the other windows as before
    X3 = X.copy()
    X3[2, 17] = np.nan
    idx3, sc3 = gpu_topk(engine, X3, G, r, 4, scores=False)
    assert (idx3[2] == -1).all() and (sc3[2] == 0).all()
    others = [0, 1, 3, 4, 5, 6, 7, 8]
    assert np.array_equal(idx3[others], idx[others]) and np.array_equal(sc3[others], sc[others])
    # every speaker NaN
    idx4, sc4 = gpu_topk(engine, X, G, np.full(S, np.nan), 2, scores=False)
    assert (idx4 == -1).all() and (sc4 == 0).all()


# ---- independence and determinism -------------------------------------------------------------------------------------------------------
def test_a_window_alone_equals_its_row_in_the_batch(engine):
    c = case(130, 300, 4, 128)
    X, G, r = c["X"], c["G"], c["r"]
    idx, sc, full = gpu_topk(engine, X, G, r, 4)
    for n in (0, 63, 64, 65, 127, 128, 129):                   # around every seam of the tiles of 64 windows
        i1, s1, f1 = gpu_topk(engine, X[n:n + 1], G, r, 4)
        assert np.array_equal(i1[0], idx[n]) and np.array_equal(s1[0], sc[n]) and np.array_equal(f1[0], full[n])
    i2, s2, f2 = gpu_topk(engine, X, G, r, 4)
    assert np.array_equal(i2, idx) and np.array_equal(s2, sc) and np.array_equal(f2, full)
    # fewer speakers: a score depends on its window and its speaker only
    i3, s3, f3 = gpu_topk(engine, X[:70], G[:100], r[:100], 4)
    assert np.array_equal(f3, full[:70, :100])
    i0, s0 = engine.plda_score_topk(dev(X[:0]), dev(G), dev(r), k=2)      # N = 0 is a no-op
    assert i0.shape == (0, 2) and s0.shape == (0, 2)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(engine):
    c = case(70, 100, 1, 128)
    X, G, r = dev(c["X"]), dev(c["G"]), dev(c["r"])
    before = gpu_topk(engine, c["X"], c["G"], c["r"], 1)
    Phi = dev(spectrum(128))
    Xp, group, n_eff = dev(c["Xp"]), dev(c["group"]), dev(c["counts"].astype(np.float64))
    bad_calls = [
        lambda: engine.plda_score_topk(X.float(), G, r),                                         # dtype
        lambda: engine.plda_score_topk(X.t().contiguous().t(), G, r),                            # contiguity
        lambda: engine.plda_score_topk(X.cpu(), G, r),                                           # device
        lambda: engine.plda_score_topk(X[:, :96].contiguous(), G[:, :192].contiguous(), r),      # D = 96
        lambda: engine.plda_score_topk(X, G, r, k=5),
        lambda: engine.plda_score_topk(X, G, r, k=0),
        lambda: engine.plda_score_topk(X, G[:0], r[:0]),                                         # S = 0
        lambda: engine.plda_score_topk(X, G, r[:50]),
        lambda: engine.plda_score_topk(X, G[:, :128].contiguous(), r),
        lambda: engine.plda_enroll(Xp.float(), group, n_eff, Phi),
        lambda: engine.plda_enroll(Xp, group.long(), n_eff, Phi),
        lambda: engine.plda_enroll(Xp, group[:-1], n_eff, Phi),
        lambda: engine.plda_enroll(Xp, group, n_eff[:0], Phi),
        lambda: engine.plda_enroll(Xp, group, n_eff, Phi[:64]),
        lambda: engine.plda_enroll(Xp[:, :96].contiguous(), group, n_eff, Phi[:96].contiguous()),
    ]
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
    # the C ABI: return code and message, shape refusals before the null context
    lib = LIB.load_library()
    st = torch.cuda.current_stream().cuda_stream
    idx = torch.full((70, 4), 77, dtype=torch.int32, device="cuda")
    sc = torch.full((70, 4), 7.5, dtype=torch.float64, device="cuda")

    def score(ctx=engine.ctx, N=70, D=128, S=100, k=1, ws=None, ws_bytes=0):
        return lib.sdk_plda_score_topk(ctx, X.data_ptr(), N, D, G.data_ptr(), r.data_ptr(), S, k, idx.data_ptr(), sc.data_ptr(), None, ws, ws_bytes, st)

    for kw, text in ((dict(D=96), "D=96 not supported"), (dict(k=5), "k=5 (1 .. 4)"), (dict(S=0), "S=0 speakers"), (dict(N=65537), "N=65537 windows"),
                     (dict(ctx=None, D=96), "D=96 not supported"), (dict(ctx=None), "null context")):
        assert score(**kw) == 2 and text in lib.sdk_last_error().decode(), (kw, lib.sdk_last_error())
    # a short workspace: 300 speakers are two splits
    G7, r7 = dev(case(130, 300, 4, 128)["G"]), dev(case(130, 300, 4, 128)["r"])
    need = lib.sdk_plda_score_workspace_bytes(70, 300, 1)
    assert need >= 2 * 70 * 4 * 12
    short = torch.empty(need - 256, dtype=torch.uint8, device="cuda")
    rc = lib.sdk_plda_score_topk(engine.ctx, X.data_ptr(), 70, 128, G7.data_ptr(), r7.data_ptr(), 300, 1, idx.data_ptr(), sc.data_ptr(), None,
                                 short.data_ptr(), short.numel(), st)
    assert rc == 2 and "workspace" in lib.sdk_last_error().decode() and str(need) in lib.sdk_last_error().decode()
    with pytest.raises(LIB.SdkError, match="workspace"):
        engine.plda_score_topk(X, G7, r7, ws=short)
    for args, text in (((70, 0, 1), "S=0"), ((70, 100, 5), "k=5"), ((-1, 100, 1), "N=-1")):
        assert lib.sdk_plda_score_workspace_bytes(*args) == 0 and text in lib.sdk_last_error().decode()
    assert lib.sdk_plda_enroll_workspace_bytes(1 << 23, 10) == 0 and "P=8388608" in lib.sdk_last_error().decode()
    rc = lib.sdk_plda_enroll(None, Xp.data_ptr(), group.data_ptr(), int(Xp.shape[0]), 96, n_eff.data_ptr(), Phi.data_ptr(), 100, G.data_ptr(),
                             r.data_ptr(), idx.data_ptr(), None, 0, st)
    assert rc == 2 and "D=96 not supported" in lib.sdk_last_error().decode()
    torch.cuda.synchronize()
    assert (idx == 77).all() and (sc == 7.5).all()                        # nothing was launched
    after = gpu_topk(engine, c["X"], c["G"], c["r"], 1)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


# ---- why pooling exists -----------------------------------------------------------------------------------------------------------------
def test_pooled_enrolments_beat_the_best_single_cosine(engine):
    """Built in float64 on the CPU.  Speaker A has ONE enrolment, close to the window; speaker B has FIVE consistent enrolments around the
    window's own centre, each farther from it than A's.  The best single cosine is A's; the by-the-book log-likelihood ratio, which knows
    that five rows pin B's centre down, prefers B."""
    d, D = 192, 128
    model = PLDA.synthetic_plda(d, 128, seed=3)
    rng = np.random.default_rng(5)

    def unit(v):
        return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)
    for trial in range(200):
        centre = rng.standard_normal(d)
        window = unit(centre + 0.9 * rng.standard_normal(d))
        a_rows = unit(window.astype(np.float64) + 1.2 / np.sqrt(d) * rng.standard_normal(d))[None]
        b_rows = unit(centre + 1.0 * rng.standard_normal((5, d)))
        P = np.concatenate([a_rows, b_rows])
        cos = P.astype(np.float64) @ window.astype(np.float64)
        Xw, Xp = model.transform_host(window[None]), model.transform_host(P)
        group = np.asarray([0, 1, 1, 1, 1, 1], np.int32)
        n_eff = np.asarray([1.0, 5.0])
        G, r, _, _ = PR.table(Xp, group, n_eff, model.Phi)
        L = PR.llr_table(Xw, G, r)[0]
        B = carried_bound(Xw, G, r, Xp, group, n_eff, model.Phi)[0]
        if np.argmax(cos) == 0 and cos[0] - cos[1:].max() > 1e-3 and L[1] - L[0] >= 10 * max(B) and L[1] - L[0] > 1e-6:
            break
    else:
        pytest.fail("no such case found")
    print(f"pooling case (trial {trial}): cosines {cos.round(4).tolist()}, llr A {L[0]:.4f}, llr B {L[1]:.4f}, bound {max(B):.2e}")
    Ed, Edb, re = engine.l2norm(dev(window[None]))
    Pn, Pb, rp = engine.l2norm(dev(P))
    cidx, _ = engine.affinity_topk(Ed, Edb, re, Pn, Pb, rp.max().reshape(1), k=1)
    Gd, rd, status = engine.plda_enroll(dev(Xp), dev(group), dev(n_eff), dev(model.Phi))
    pidx, psc = engine.plda_score_topk(dev(Xw), Gd, rd, k=2)
    torch.cuda.synchronize()
    assert int(cidx[0, 0]) == 0                                           # the cosine takes A's row
    assert pidx[0].tolist() == [1, 0] and int(status.item()) == 0         # the pooled score takes B
    assert abs(float(psc[0, 0]) - L[1]) <= B[1] and abs(float(psc[0, 1]) - L[0]) <= B[0]


# ---- the Backend end to end -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", ["1", "0"])
def test_backend_identifies_on_the_llr_scale_and_is_untouched_without_a_model(tmp_path, monkeypatch, count):
    """Synthetic weights, a synthetic PLDA of the family's width written by save_plda, the stand-in voices of evals/run_eval.py.  The reference
    reads the DEVICE's own transformed rows (windows and profiles), so what separates the two sides is the enrolment arithmetic (enrol_bounds,
    carried into a score as |x| bG + x^2 bq + br) and the scoring arithmetic (score_bound)."""
    sys.path.insert(0, str(ROOT / "evals"))
    from run_eval import render_voice
    wav, store, BK, PS = sub("wav"), sub("store"), sub("backend"), sub("plda_score")
    monkeypatch.setenv("SPEAKERS_EMBEDDINGS_DIR", str(tmp_path / "store"))
    monkeypatch.setenv("SDK_CACHE_DIR", str(tmp_path / "cache"))
    for v in ("SDK_COHORT", "SDK_COHORT_THRESHOLD", "SDK_NO_TORCH", "SDK_SCORE_PLDA_DIM", "SDK_SCORE_PLDA_THRESHOLD"):
        monkeypatch.delenv(v, raising=False)
    tnpz, pnpz = tmp_path / "xvec_transform.npz", tmp_path / "plda.npz"
    monkeypatch.setenv("SDK_SCORE_PLDA_TRANSFORM", str(tnpz))
    monkeypatch.setenv("SDK_SCORE_PLDA", str(pnpz))
    monkeypatch.setenv("SDK_SCORE_PLDA_COUNT", count)
    be = BK.Backend()
    d = be.embedding_dim
    model = PLDA.synthetic_plda(d, 128)
    PLDA.save_plda(model, tnpz, pnpz)
    assert be.plda_scoring and np.array_equal(be.score_plda().Phi, model.Phi)

    def recording(name, tags, seconds, seed):
        path = tmp_path / f"{name}.wav"
        wav.write_wav_s16(path, np.concatenate([render_voice(t, seconds, seed + 11 * j) for j, t in enumerate(tags)]))
        return path

    profiles = []
    for i, (sid, takes) in enumerate((("ann", 2), ("bob", 1), ("cy", 1))):           # ann owns two embeddings
        embs = []
        for t in range(takes):
            rec = be.enroll_speaker(recording(f"enroll_{sid}_{t}", [sid], 5.0, 100 + 7 * i + 50 * t))
            embs.append({"id": f"emb-{sid}-{t}", "external_id": rec["external_id"], "model_version": rec["model_version"], "trust_level": "high"})
        profiles.append({"id": sid, "names": {"default": sid.title()}, "embeddings": {"mi355x": embs}})
    meeting = recording("meeting", ["bob", "ann", "stranger"], 4.0, 300)
    second = recording("second", ["cy", "ann"], 3.0, 400)

    def reference(path, cands):
        batch = store.load_profile_batch(cands, "mi355x", model_prefix="mi355x-")
        samples, starts, W, spans = be._windows(path, None)
        Ed = be.embed_tables(samples, {W: starts})[W][0]
        Xw = be._plda_rows(Ed).cpu().numpy()
        Xp = be._plda_rows(be.profile_tensors(batch)[0]).cpu().numpy()
        group, speakers, first, counts = PS.group_speakers(batch.speaker_ids)
        n_eff = counts.astype(np.float64) if count == "1" else np.ones(len(speakers))
        G, r, _, _ = PR.table(Xp, group, n_eff, model.Phi)
        L = PR.llr_table(Xw, G, r)
        B = carried_bound(Xw, G, r, Xp, group, n_eff, model.Phi)
        didx, dllr = (a[:, 0] for a in be.score_windows_plda(Ed, batch))
        n = np.arange(len(Xw))
        assert (didx >= 0).all() and (didx < len(speakers)).all()
        lsel, bsel = L[n, didx], B[n, didx]
        assert (np.abs(dllr - lsel) <= bsel).all()
        assert ((L - B).max(axis=1) <= lsel + bsel).all(), "the device's winner must be one the bound allows"
        print(f"e2e plda {path.name} count={count}: {len(Xw)} windows x {len(speakers)} speakers of {counts.tolist()} embeddings, "
              f"worst |llr - ref| / bound {float((np.abs(dllr - lsel) / bsel).max()):.4f}, worst bound {float(B.max()):.3e}")
        return batch, didx, lsel, bsel, L.max(axis=1), spans

    def same_rows(rows, want, b):
        assert rows == sorted(rows, key=lambda r: (-r["llr"], r["speaker_id"]))
        assert sorted(r["speaker_id"] for r in rows) == sorted(r["speaker_id"] for r in want)
        by = {r["speaker_id"]: r for r in rows}
        for w in want:
            r = by[w["speaker_id"]]
            assert set(r) == {"speaker_id", "llr", "similarity", "confidence", "embedding_id", "n_embeddings", "segment", "n_segments"}
            assert all(r[f] == w[f] for f in ("n_segments", "embedding_id", "n_embeddings", "segment"))
            assert abs(r["llr"] - w["llr"]) <= b and r["similarity"] == r["confidence"] == PS.confidence(r["llr"])
        for x, y in zip(want, want[1:]):
            if x["llr"] - y["llr"] > 2 * b:
                assert [r["speaker_id"] for r in rows].index(x["speaker_id"]) < [r["speaker_id"] for r in rows].index(y["speaker_id"])

    batch, idx, llr, b, top, spans = reference(meeting, profiles)
    ts = np.sort(top)
    g = int(np.argmax(np.diff(ts)))
    thr = float(0.5 * (ts[g] + ts[g + 1]))
    print(f"e2e plda: top-1 llr per window {top.round(3).tolist()}, threshold {thr:.4f} in a gap of {ts[g + 1] - ts[g]:.4f}, "
          f"least |llr - threshold| / bound {float((np.abs(llr - thr) / b).min()):.3g}")
    assert len(llr) >= 6 and (np.abs(llr - thr) >= 2 * b).all(), "every window's vote must be decided: twice its bound away from the threshold"
    assert (llr >= thr).any() and (llr < thr).any()
    be.score_plda_threshold = thr
    want = PR.aggregate(idx, llr, spans, batch.speaker_ids, batch.embedding_ids, thr)
    rows = be.identify_speaker(meeting, profiles, threshold=0.99)          # the raw threshold is not applied on this path
    assert len(want) >= 1
    same_rows(rows, want, float(b.max()))
    ann = [r for r in rows if r["speaker_id"] == "ann"]
    assert all(r["embedding_id"] == "emb-ann-0" and r["n_embeddings"] == 2 for r in ann)
    cached = getattr(be.last_batch, "_plda")
    assert cached[1] == (be._score_plda[1], count == "1")
    many = be.identify_many([meeting, second], profiles)
    assert many == [rows, be.identify_speaker(second, profiles)]
    got = be.verify_speaker(meeting, profiles[0])
    hit = be.identify_speaker(meeting, [profiles[0]])
    if hit:
        assert got == {"match": True, "similarity": hit[0]["similarity"], "confidence": hit[0]["similarity"], "embedding_id": "emb-ann-0",
                       "llr": hit[0]["llr"]}
    else:
        assert got == {"match": False, "similarity": 0.0, "confidence": 0.0, "embedding_id": None}
    vb, vidx, vllr, vbb, _, vspans = reference(meeting, [profiles[0]])
    if (np.abs(vllr - thr) > vbb).all():
        same_rows(hit, PR.aggregate(vidx, vllr, vspans, vb.speaker_ids, vb.embedding_ids, thr), float(vbb.max()))

    # with the variables unset the raw path answers as before: score_windows + aggregate_matches on the same embeddings
    for v in ("SDK_SCORE_PLDA_TRANSFORM", "SDK_SCORE_PLDA", "SDK_SCORE_PLDA_COUNT"):
        monkeypatch.delenv(v, raising=False)
    plain = BK.Backend()
    assert not plain.plda_scoring and plain.score_plda() is None
    samples, starts, W, spans = plain._windows(meeting, None)
    E, Eb, re = plain.embed_tables(samples, {W: starts})[W]
    b2 = store.load_profile_batch(profiles, "mi355x", model_prefix="mi355x-")
    pidx, psc = plain.score_windows(E, Eb, re, b2)
    before = BK.aggregate_matches(pidx[:, 0], psc[:, 0], spans, b2, 0.354)
    now = plain.identify_speaker(meeting, profiles, threshold=0.354)
    assert now == before and all("llr" not in r and "n_embeddings" not in r for r in now)
    assert getattr(plain.last_batch, "_plda", None) is None
