"""CPU checks of the fixtures of tests/test_vbx_edges_gpu.py, which also holds nothing of its own: the cases, their inputs and their reference runs
are built here and imported there.

A. The iteration kernels (sdk_vbx, sdk_vbx_hmm) at the sizes where csrc/vbx.hip changes its path: the chain's speaker registers per lane
   (K = ceil(S / 64), the memory form above 256), a full and a one-lane top register, the chain's two prefetch buffers of four rows (a trip of the
   unrolled loop takes eight steps; the last trip takes (n - 1) mod 8 of them), the E step's groups of four rows (nr = min(4, n - ta)) and the
   statistics kernel's chunks of 16 speakers (ns = min(16, S - s0)).  Every case runs two iterations with epsilon = -inf: n_iter is 2 by construction,
   no stop decision exists, and iteration 2 reads the pi that iteration 1 wrote.  Only gamma, pi and the ELBO are compared, so no speaker weight
   near the keep threshold can break a fixture (with S >> n tens of them lie there).  What a case claims to reach is written out by hand below
   (S_PATH, N_PATH); the tests recompute it by walking the kernels' loops over the indices, and assert that the list as a whole still covers every
   path, so a later edit of the list cannot drop one silently.  n = 7 is in the list for that reason: without it no case of four registers or of
   the memory form ends its last trip after six steps.
   One case takes the third yardstick term that tests/vbx_hmm_ref.py provides, a float64 run with every exp, log and log1p moved by one ulp
   (JITTER): n = 18, S = 17, D = 128 at loop_prob 0.  There the two summation-order runs happen to move pi by 3.5e-15 only, while they move gamma,
   whose column means pi is, by 7.9e-14; the device's pi lay 2.9e-14 from the reference, 8.2 x that yardstick, and its gamma 2.2 x its own.  The
   margin stays 8.
B. sdk_vbx_centroids on inputs built here, so that every decision is exact by design: the margins of the row maxima, one planted tie, speaker
   weights far from the keep threshold.  The tests assert those construction conditions."""
from __future__ import annotations

import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import partial_width as PW  # noqa: E402
import test_vbx_hmm_gpu as HG  # noqa: E402  (its mixture and yardstick; importing it needs no GPU)
import vbx_hmm_ref as HR  # noqa: E402
import vbx_ref as VR  # noqa: E402

RUNS = (("f64", np.float64, False), ("ld", np.longdouble, False), ("rev", np.float64, True))

# ------------------------------------------------------------------------------------------------ A: the cases
N_LIST = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13, 16, 17, 18]
N_BLOCK = [64, 65]                                                        # the 64-row block edge, with four registers and the memory form: loop_prob 0.9 only
S_BLOCK = (193, 256, 257)
SD = [(16, 64), (17, 64), (17, 128), (32, 64), (64, 64), (128, 64), (129, 64), (192, 64), (193, 64), (193, 128), (256, 64), (257, 64)]
ENTRIES = [None, 0.0, 0.9]                                                # sdk_vbx; sdk_vbx_hmm at these loop probabilities
ITERS = 2
JITTER = {((18, 128, 17, 3), 0.0): 100 + 18 + 17}                         # (case, entry) -> the seed of its one-ulp run (the seed of its mixture)

# what a size claims to reach, by hand.  S -> (speaker registers per lane or "memory", live lanes of the top register, the chunk sizes ns)
S_PATH = {16: (1, 16, {16}), 17: (1, 17, {16, 1}), 32: (1, 32, {16}), 64: (1, 64, {16}), 128: (2, 64, {16}), 129: (3, 1, {16, 1}), 192: (3, 64, {16}),
          193: (4, 1, {16, 1}), 256: (4, 64, {16}), 257: ("memory", None, {16, 1})}
# n -> (steps of the chain's last trip, 0 for a full one of eight; the group sizes nr)
N_PATH = {1: (0, {1}), 2: (1, {2}), 3: (2, {3}), 4: (3, {4}), 5: (4, {4, 1}), 6: (5, {4, 2}), 7: (6, {4, 3}), 8: (7, {4}), 9: (0, {4, 1}), 10: (1, {4, 2}),
          13: (4, {4, 1}), 16: (7, {4}), 17: (0, {4, 1}), 18: (1, {4, 2}), 64: (7, {4}), 65: (0, {4, 1})}


def cases_of(S, D):
    """The (case, entry) pairs of one (S, D): case = (n, D, S, true speakers) as test_vbx_hmm_gpu.mixture takes it."""
    out = [((n, D, S, min(3, n)), e) for n in N_LIST for e in ENTRIES]
    if S in S_BLOCK and D == 64:
        out += [((n, D, S, 3), 0.9) for n in N_BLOCK]
    return out


_X, _runs = {}, {}


def edge_runs(case, entry):
    """The three reference runs of one case and entry (computed once, shared, never changed): gamma, pi, elbo, n_iter of each."""
    key = (case, entry)
    if key not in _runs:
        n, D, S, _ = case
        m, E, rows, init, _ = HG.mixture(case)
        out = {}
        for name, dt, rev in RUNS:
            if (case, dt) not in _X:
                _X[case, dt] = VR.transform(E[rows], m.mean1, m.lda, m.mean2, m.mu, m.T, dt)
            kw = dict(epsilon=-np.inf, max_iters=ITERS, dtype=dt, reverse=rev)
            r = VR.vbx(_X[case, dt], m.Phi, init, S, **kw) if entry is None else HR.vbx_hmm(_X[case, dt], m.Phi, init, S, entry, **kw)
            out[name] = dict(gamma=r["gamma"], pi=r["pi"], elbo=r["elbo"], n_iter=r["n_iter"])
        if key in JITTER:
            r = HR.vbx_hmm(_X[case, np.float64], m.Phi, init, S, entry, epsilon=-np.inf, max_iters=ITERS, jitter=JITTER[key])
            out["ulp"] = dict(gamma=r["gamma"], pi=r["pi"], elbo=r["elbo"], n_iter=r["n_iter"])
        _runs[key] = out
    return _runs[key]


# ------------------------------------------------------------------------------------------------ A: the kernels' index arithmetic, walked
VH_PF, VH_MAXK, VB_ROWS, VB_SC = 4, 4, 64, 16


def chain_form(S):
    """vbx_chain_launch -> (K or "memory", the lanes of the top register with lane + 64 (K - 1) < S)."""
    K = (S + 63) // 64
    if K > VH_MAXK:
        return "memory", None
    return K, sum(lane + 64 * (K - 1) < S for lane in range(64))


def chain_trips(n):
    """vbx_chain_kernel's two loops -> per direction the rows stepped, and per trip the steps taken from buffer A and from buffer B."""
    fwd, ftrips = [], []
    for t0 in range(1, n, 2 * VH_PF):
        a = [t0 + j for j in range(VH_PF) if t0 + j < n]
        b = [t0 + VH_PF + j for j in range(VH_PF) if t0 + VH_PF + j < n]
        fwd += a + b
        ftrips.append((len(a), len(b)))
    bwd, btrips = [], []
    for t0 in range(n - 2, -1, -2 * VH_PF):
        a = [t0 - j for j in range(VH_PF) if t0 - j >= 0]
        b = [t0 - VH_PF - j for j in range(VH_PF) if t0 - VH_PF - j >= 0]
        bwd += a + b
        btrips.append((len(a), len(b)))
    return fwd, ftrips, bwd, btrips


def estep_groups(n):
    """vbx_estep_kernel -> the nr of every group of four rows that a wave takes."""
    out = []
    for blk in range((n + VB_ROWS - 1) // VB_ROWS):
        for wave in range(4):
            for q in range(4):
                ta = blk * VB_ROWS + wave * 16 + q * 4
                if ta >= n:
                    break
                out.append(min(4, n - ta))
    return out


def stats_chunks(S):
    """vbx_stats_kernel's grid.y -> the ns of every chunk."""
    return [min(VB_SC, S - c * VB_SC) for c in range((S + VB_SC - 1) // VB_SC)]


@pytest.mark.parametrize("S", sorted(S_PATH))
def test_a_speaker_count_reaches_the_path_it_claims(S):
    K, lanes, ns = S_PATH[S]
    assert chain_form(S) == (K, lanes) and set(stats_chunks(S)) == ns and sum(stats_chunks(S)) == S
    assert (K == "memory") == (S > 256) and (K == "memory" or K == -(-S // 64))
    assert ns == {16} | ({S % 16} - {0})


@pytest.mark.parametrize("n", sorted(N_PATH))
def test_a_row_count_reaches_the_path_it_claims(n):
    last, nr = N_PATH[n]
    fwd, ftrips, bwd, btrips = chain_trips(n)
    assert fwd == list(range(1, n)) and bwd == list(range(n - 2, -1, -1))            # every row once, in order
    assert ftrips == btrips and last == (n - 1) % 8
    if n > 1:
        assert sum(ftrips[-1]) == (last or 8) and all(t == (4, 4) for t in ftrips[:-1]) and len(ftrips) == -(-(n - 1) // 8)
        assert ftrips[-1] == (min(4, last or 8), max(0, (last or 8) - 4))             # buffer A first; B only past four steps
    g = estep_groups(n)
    assert set(g) == nr and sum(g) == n and nr == ({4} if n >= 4 else set()) | ({n % 4} - {0})


def test_the_cases_cover_every_path():
    assert all(e is not None and (c, e) in cases_of(c[2], c[1]) for c, e in JITTER)      # the one-ulp run exists for the chain only
    sizes = {(S, D) for S, D in SD}
    assert {S for S, _ in sizes} == set(S_PATH) and {(17, 128), (193, 128)} <= sizes
    pairs = {(c[0], c[2]) for S, D in SD for c, _ in cases_of(S, D)}
    assert all(n in N_PATH and S in S_PATH for n, S in pairs)
    forms = {S_PATH[S][0] for _, S in pairs}
    assert forms == {1, 2, 3, 4, "memory"}
    assert {S_PATH[S][1] for _, S in pairs if S_PATH[S][0] == 4} >= {1, 64}          # four registers: a one-lane and a full top register
    for form in (4, "memory"):
        assert {N_PATH[n][0] for n, S in pairs if S_PATH[S][0] == form and n > 1} == set(range(8)), form
        assert {n for n, S in pairs if S_PATH[S][0] == form} >= {64, 65}              # the 64-row block edge
    for K in (1, 2, 3, 4):
        assert any(S_PATH[S][0] == K and S_PATH[S][1] == 64 for _, S in pairs), K     # a full register at every K
    assert set().union(*(N_PATH[n][1] for n, _ in pairs)) == {1, 2, 3, 4}
    assert set().union(*(S_PATH[S][2] for _, S in pairs)) == {1, 16}
    assert {256, 257} <= {S for _, S in pairs} and {1, 16, 17} <= {n for n, _ in pairs}
    # the entries: sdk_vbx (whose E step is the LOGP = false form) meets n = 1 and a wave's slice ending at rows 16 and 17
    for S, D in SD:
        got = {(c[0], e) for c, e in cases_of(S, D)}
        assert {(n, e) for n in (1, 16, 17) for e in ENTRIES} <= got


@pytest.mark.parametrize("S,D", SD, ids=lambda v: str(v))
def test_the_reference_runs_of_a_size_are_sound(S, D):
    for case, entry in cases_of(S, D):
        n = case[0]
        runs = edge_runs(case, entry)
        for name in runs:
            r = runs[name]
            assert r["n_iter"] == ITERS and r["gamma"].shape == (n, S) and r["pi"].shape == (S,) and r["elbo"].shape == (ITERS,), (case, entry, name)
            assert all(np.isfinite(np.asarray(r[q], np.float64)).all() for q in ("gamma", "pi", "elbo")), (case, entry, name)
        for q in ("gamma", "pi", "elbo"):
            y = HG.yardstick(runs, q)
            assert np.isfinite(y), (case, entry, q)
        g = runs["f64"]["gamma"]
        assert np.abs(g.sum(1) - 1.0).max() <= 1e-12 and abs(runs["f64"]["pi"].sum() - 1.0) <= 1e-12


# ------------------------------------------------------------------------------------------------ B: the inputs of sdk_vbx_centroids
# the last two: a thread's second column (j1 = tid + 256) live for wave 0 only (d = 320) and for every wave but the last (448), one row past the tile
CENTROID_SHAPES = [(1, 1, 64), (255, 5, 320), (256, 5, 512), (257, 70, 512), (513, 3, 384), (300, 7, 256), (257, 3, 320), (257, 5, 448)]
NONE_KEPT = (257, 5, 320)
MIN_PI = 1e-7
MARGIN_OF_MAXIMA = 0.05
_cent = {}


def roles(S):
    """What each speaker is: "kept", "zero" (kept, its gamma column all zero), or dropped with pi = 1e-12 ("tiny"), 0.0 ("null") or NaN ("nan").
    S = 1 has its one kept speaker; S = 3 a dropped one between two kept (no room for the zero column beside the tie); from S = 5 on everything."""
    if S < 5:
        return {1: ["kept"], 3: ["kept", "tiny", "kept"]}[S]
    tail = itertools.cycle(["null", "kept", "kept", "tiny", "kept", "nan"])
    return ["kept", "tiny", "zero", "nan", "kept"] + [next(tail) for _ in range(S - 5)]


def centroid_case(shape):
    """-> dict(E [R, d] unit fp32 rows, rows [n] ascending strict subset, gamma [n, S], pi [S], roles, tie (row, lower column, upper column) or None).
    A row of gamma: its largest entry, 0.55 .. 0.6, in any column that is not the zero one, a dropped speaker's included; its second, 0.27 .. 0.3, in a
    kept column; the rest, 0.1 .. 0.18 in all, spread over the other columns.  So the maximum leads by 0.25 and more, and among the kept columns
    alone the leader leads by 0.09 and more.  The tie row holds 0.4 twice."""
    if shape not in _cent:
        n, S, d = shape
        rng = np.random.default_rng(1000 + n + 7 * S + d)
        R = n + max(3, n // 5)
        E = rng.standard_normal((R, d))
        E = (E / np.linalg.norm(E, axis=1, keepdims=True)).astype(np.float32)
        rows = np.sort(rng.choice(R, n, replace=False)).astype(np.int32)
        role = roles(S)
        live = [s for s in range(S) if role[s] == "kept"]
        nz = [s for s in range(S) if role[s] != "zero"]
        pi = np.array([dict(tiny=1e-12, null=0.0, nan=np.nan, zero=0.5).get(r, 0.0) for r in role])
        pi[live] = 10.0 ** rng.uniform(-3.0, 0.0, len(live))
        pi[live[0]], pi[live[-1]] = 1e-3, 1.0                             # the ends of the range, exactly (S = 1: 1.0)
        gamma = np.zeros((n, S))
        tie = None
        for t in range(n):
            if len(nz) == 1:
                gamma[t, nz[0]] = 1.0
                continue
            c1 = int(rng.choice(nz))
            c2 = int(rng.choice([s for s in live if s != c1]))
            a, b = rng.uniform(0.55, 0.6), rng.uniform(0.27, 0.3)
            rest = [s for s in nz if s not in (c1, c2)]
            w = rng.random(len(rest)) + 0.1
            gamma[t, rest] = (1.0 - a - b) * w / w.sum()
            gamma[t, c1], gamma[t, c2] = a, b
        if n > 1 and len(live) > 1:
            t, k1, k2 = n // 2, live[1] if len(live) > 2 else live[0], live[-1]
            rest = [s for s in nz if s not in (k1, k2)]
            w = rng.random(len(rest)) + 0.1
            gamma[t] = 0.0
            gamma[t, rest] = 0.2 * w / w.sum()
            gamma[t, k1] = gamma[t, k2] = 0.4
            tie = (t, k1, k2)
        _cent[shape] = dict(E=E, rows=rows, gamma=gamma, pi=pi, roles=role, tie=tie)
    return _cent[shape]


def centroid_runs(shape):
    """vbx_ref.result on one case in float64, long double and with the rows descending (computed once, shared)."""
    c = centroid_case(shape)
    if "runs" not in c:
        c["runs"] = {name: VR.result(c["gamma"], c["pi"], c["E"][c["rows"]], dt, rev) for name, dt, rev in RUNS}
    return c["runs"]


def centroid_tolerance(shape):
    """-> (yardstick, tolerance) of cent64: MARGIN x the larger distance of the float64 run to its long-double and its descending run + ULPS ulp."""
    runs = centroid_runs(shape)
    want = runs["f64"]["cent"]
    y = max(float(np.abs(want.astype(np.longdouble) - runs[k]["cent"].astype(np.longdouble)).max()) for k in ("ld", "rev"))
    return y, HG.MARGIN * y + HG.ULPS * float(np.spacing(np.abs(want).max()))


def centroid_weight(shape) -> float:
    """partial_width.weight of a centroid case wider than 256: vbx_ref.result without the columns 256.. of the rows (the labels come from gamma
    alone, so only the centroids can move)."""
    c = centroid_case(shape)
    ref = centroid_runs(shape)["f64"]
    cut = VR.result(c["gamma"], c["pi"], PW.first_columns(c["E"][c["rows"]]))
    return PW.weight("vbx centroids n=%d S=%d d=%d" % shape, ints=[(ref["keep"], cut["keep"])], floats=[(ref["cent"], cut["cent"])], bound=centroid_tolerance(shape)[1])


def none_kept_case():
    """NONE_KEPT's inputs with every speaker weight at 0 or 1e-12: K = 0."""
    c = dict(centroid_case(NONE_KEPT))
    c["pi"] = np.where(np.arange(NONE_KEPT[1]) % 2 == 0, 0.0, 1e-12)
    c.pop("runs", None)
    return c


@pytest.mark.parametrize("shape", CENTROID_SHAPES, ids=lambda s: "n%d-S%d-d%d" % s)
def test_the_centroid_inputs_are_what_they_claim(shape):
    n, S, d = shape
    c = centroid_case(shape)
    E, rows, gamma, pi, role, tie = (c[k] for k in ("E", "rows", "gamma", "pi", "roles", "tie"))
    assert E.dtype == np.float32 and E.shape[1] == d and np.abs(np.linalg.norm(E.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    assert rows.dtype == np.int32 and len(rows) == n < E.shape[0] and (np.diff(rows) > 0).all() and rows.min() >= 0 and rows.max() < E.shape[0]
    assert gamma.shape == (n, S) and (gamma >= 0).all() and np.abs(gamma.sum(1) - 1.0).max() <= 1e-14
    # the speaker weights: 0, 1e-12, NaN or 1e-3 .. 1, so none within a factor 1e4 of the keep threshold
    fin = pi[~np.isnan(pi)]
    assert ((fin == 0.0) | (fin == 1e-12) | ((fin >= MIN_PI * 1e4) & (fin <= 1.0))).all()
    kept = [s for s in range(S) if pi[s] > MIN_PI]
    assert kept == [s for s in range(S) if role[s] in ("kept", "zero")]
    # the row maxima: over all columns and over the kept columns alone, but for the planted tie
    free = np.ones(n, bool)
    if tie is not None:
        t, k1, k2 = tie
        free[t] = False
        assert k1 < k2 and k1 in kept and k2 in kept and gamma[t, k1] == gamma[t, k2] == gamma[t].max()
        assert np.sort(gamma[t])[-3] <= gamma[t, k1] - MARGIN_OF_MAXIMA
    for cols in (np.arange(S), np.array(kept)):
        if len(cols) > 1:
            g = np.sort(gamma[free][:, cols], axis=1)
            assert (g[:, -1] - g[:, -2]).min() >= MARGIN_OF_MAXIMA
    runs = centroid_runs(shape)
    ref = runs["f64"]
    assert all(np.array_equal(runs[k]["keep"], kept) and np.array_equal(runs[k]["labels"], ref["labels"]) for k in runs)
    assert all(np.isfinite(np.asarray(runs[k]["cent"], np.float64)).all() for k in runs)
    if tie is not None:
        assert ref["labels"][tie[0]] == kept.index(tie[1])                               # to the lower of the two
    if S >= 3:
        dropped = [s for s in range(S) if s not in kept]
        assert any(kept[0] < s < kept[-1] for s in dropped)
        assert S < 5 or {"tiny", "nan"} <= set(role) and (S == 5 or "null" in role)
        assert (gamma[:, dropped].max(0) > 0.5).any()                                    # a dropped column holds some row's maximum
    if S >= 5:
        z = role.index("zero")
        assert z in kept and not gamma[:, z].any() and not ref["cent"][kept.index(z)].any() and kept.index(z) not in ref["labels"]
        live = [kept.index(s) for s in kept if s != z]
        assert np.abs(np.linalg.norm(ref["cent"][live].astype(np.float64), axis=1) - 1.0).max() < 1e-12
    else:
        assert "zero" not in role
    assert all((gamma[:, s] > 0).any() for s in kept if role[s] == "kept")
    if d > PW.FIRST:
        assert centroid_weight(shape) > PW.FAR


def test_the_shapes_cover_the_centroid_kernels_edges():
    assert {d > 256 for _, _, d in CENTROID_SHAPES} == {True, False} and max(d for _, _, d in CENTROID_SHAPES) == 512      # the second column per thread
    assert {d for n, _, d in CENTROID_SHAPES if n == 257} >= set(PW.WIDTHS)               # .. live for one wave, and for all but one, past the row tile
    assert {n for n, _, _ in CENTROID_SHAPES} >= {1, 255, 256, 257, 513}                  # the 256-row LDS tile: below, exact, one over, two tiles and one
    assert any(S > 64 for _, S, _ in CENTROID_SHAPES)
    assert sum("zero" in roles(S) for _, S, _ in CENTROID_SHAPES) >= 3 and sum("nan" in roles(S) for _, S, _ in CENTROID_SHAPES) >= 3
    c = none_kept_case()
    assert not (c["pi"] > MIN_PI).any() and (c["pi"] <= 1e-12).all() and set(c["pi"].tolist()) == {0.0, 1e-12}
    r = VR.result(c["gamma"], c["pi"], c["E"][c["rows"]])
    assert len(r["keep"]) == 0 and r["cent"].shape == (0, NONE_KEPT[2]) and (r["labels"] == -1).all()


# ------------------------------------------------------------------------------------------------ C: sdk_plda_transform with two partial second columns
TRANSFORM_CASE = (9, 320, 300, 128)               # n rows of a 12-row table, d_in, D0, D: the second column partial over d_in AND over D0
_transform = {}


def transform_case():
    """-> dict(m the synthetic model, E [12, d_in] unit fp32 rows, rows [n] ascending strict subset, f64 / ld: vbx_ref.transform of the rows)."""
    if not _transform:
        n, d_in, D0, D = TRANSFORM_CASE
        m = HG.P.synthetic_plda(d_in, D0, seed=d_in + D0, lda_dim=D)
        rng = np.random.default_rng(d_in + D0 + n)
        E = rng.standard_normal((n + 3, d_in))
        E = (E / np.linalg.norm(E, axis=1, keepdims=True)).astype(np.float32)
        rows = np.sort(rng.choice(n + 3, n, replace=False)).astype(np.int32)
        _transform.update(m=m, E=E, rows=rows, **{k: VR.transform(E[rows], m.mean1, m.lda, m.mean2, m.mu, m.T, dt) for k, dt in (("f64", np.float64), ("ld", np.longdouble))})
    return _transform


def transform_tolerance():
    c = transform_case()
    y = float(np.abs(c["f64"].astype(np.longdouble) - c["ld"]).max())
    return y, HG.MARGIN * y + HG.ULPS * float(np.spacing(np.abs(c["f64"]).max()))


def test_the_transform_case_has_two_partial_second_columns_and_weighs_them():
    n, d_in, D0, D = TRANSFORM_CASE
    c = transform_case()
    m = c["m"]
    assert PW.FIRST < D0 < d_in < 512 and d_in in PW.WIDTHS and D0 % 64 and m.lda.shape == (d_in, D0) and m.T.shape == (D, D0)
    assert c["f64"].shape == (n, D) and np.isfinite(c["f64"]).all() and len(c["rows"]) == n < len(c["E"])
    y, tol = transform_tolerance()
    # without the input columns 256.., and without the intermediate columns 256.. of x2 (the rows of T^T the second output column of a thread reads)
    cut = VR.transform(PW.first_columns(c["E"][c["rows"]]), m.mean1, m.lda, m.mean2, m.mu, m.T)
    assert PW.weight(f"plda transform {d_in} -> {D0} -> {D}, input columns", floats=[(c["f64"], cut)], bound=tol) > PW.FAR
    cut = VR.transform(c["E"][c["rows"]], m.mean1, PW.first_columns(m.lda), PW.first_columns(m.mean2), PW.first_columns(m.mu), m.T)
    assert PW.weight(f"plda transform {d_in} -> {D0} -> {D}, D0 columns", floats=[(c["f64"], cut)], bound=tol) > PW.FAR
