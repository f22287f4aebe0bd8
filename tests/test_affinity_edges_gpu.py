"""sdk_affinity_topk pinned to its exact fp32 scan, BIT FOR BIT, on every path and at every edge; sdk_l2norm at its edges.

The header of csrc/scoring.hip promises that the reported (idx, score) equal an fp32 full scan computed with one fixed dot-product routine,
whichever kernel computed them, ties to the lower profile index.  tests/affinity_ref.py restates that routine on the host with a correctly
rounded fma, so every comparison here is np.array_equal on the index and on the score's BITS, against the restatement applied to the device's
OWN sdk_l2norm output rows.  No tolerance, no mismatch allowance.

Paths (engine options, restored in `finally`: the engine is session-wide):
    fast        default, k = 1: the row/column kernel under its cost model (P <= 32768; beyond it the default k = 1 call IS the general kernel)
    range       affinity_variant 7: the range plan
    b8/b12/b13  affinity_variant 8 / 12 / 13: the block plan with 1 / 2 / 3 records where sdk_affinity_block_plan says the shape has one
                (N >= 8 * 32 * compute units: the case N = 65569 below); every other shape falls back to the range plan and is compared too
    gen1        affinity_fast_path 0, k = 1: affinity_coarse_kernel<3> (P <= 2048) / <4>
    gen2..gen4  k = 2, 3, 4: depth 3 for k <= 2 and P <= 2048, depth 4 otherwise
P = 32769 and 33000 give 33 rescan slices = 132 > 128 partial entries: affinity_rescan_merge_kernel takes its second pass for every rescanned row.
"""
import numpy as np
import pytest
import torch

import affinity_ref as R
from conftest import sub

pytestmark = pytest.mark.gpu

# (kind, N, P, seed).  N edges: 1; 31 / 32 / 33 (rescore block, block-plan group); 127 / 128 / 129 (segments per workgroup of the general kernel);
# 513 (past the range plan's 512-segment group).  P edges: 1 - 4 (k == P); 31 / 32 / 33 and 63 / 64 / 65 (tile, stage of two tiles); 1023 / 1024 /
# 1025 (10-bit index chunk, rescan slice); 2048 / 2049 (depth 3 -> 4); 32768 (last P of the fast path) / 32769 / 33000 (general kernel for k = 1, 33
# slices).  N <= 33 wherever P > 4096.  N = 65569 = 8 * 32 * 256 + 33 is the smallest N with a block plan on 256 compute units (two leftover blocks,
# swept in three parts); P = 353 there = 6 stages, so that 2 and 3 records per sweep exist, with a partial last tile.
_GAUSS = [(1, 1), (33, 1), (31, 2), (128, 2), (32, 3), (129, 3), (127, 4), (513, 4), (1, 31), (129, 31), (33, 32), (128, 32), (32, 33), (513, 33),
          (31, 63), (127, 63), (128, 64), (33, 64), (129, 65), (1, 65), (32, 1023), (127, 1023), (128, 1024), (513, 1024), (33, 1025), (129, 1025),
          (31, 2048), (128, 2048), (127, 2049), (513, 2049), (1, 32768), (33, 32768), (32, 32769), (33, 32769), (31, 33000), (33, 33000)]
_KNOTS = [(33, 33), (129, 65), (1, 1025), (513, 1025), (31, 2048), (128, 2049), (1, 32768), (33, 32768), (32, 32769), (1, 33000), (33, 33000),
          (65569, 353)]
_DUPS = [(33, 33), (1, 1025), (128, 1025), (513, 2049), (33, 32769), (32, 33000)]
_ENDS = [(1, 31), (1, 63), (33, 33), (129, 65), (127, 1023), (32, 1025), (513, 2049), (31, 32769), (33, 33000)]
_NEG = [(33, 31), (128, 64), (513, 1025), (127, 2049), (33, 32768), (32, 32769)]
_ZEROS = [(33, 32, 0), (1, 33, 0), (1, 33, 1), (129, 1024, 1), (32, 2049, 0), (1, 32768, 0), (31, 32769, 1), (5, 3, 0)]
FIXTURES = ([("gauss", N, P, 0) for N, P in _GAUSS] + [("knots", N, P, 0) for N, P in _KNOTS] + [("dups", N, P, 0) for N, P in _DUPS]
            + [("ends", N, P, s) for s, (N, P) in enumerate(_ENDS)] + [("negative", N, P, 0) for N, P in _NEG]
            + [("zeros", N, P, s) for N, P, s in _ZEROS])

K1_PATHS = [("fast", {}), ("range", {"affinity_variant": 7}), ("b8", {"affinity_variant": 8}), ("b12", {"affinity_variant": 12}),
            ("b13", {"affinity_variant": 13}), ("gen1", {"affinity_fast_path": 0})]
RESET = {"affinity_variant": 0, "affinity_fast_path": 1}


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _norm(engine, X):
    E, Eb, r = engine.l2norm(torch.from_numpy(np.ascontiguousarray(X)).cuda())
    return E, Eb, r


def _call(engine, e, p, rp_max, k, opts):
    try:
        for name, v in opts.items():
            engine.set_option(name, v)
        idx, sc, cnt = engine.affinity_topk(e[0], e[1], e[2], p[0], p[1], rp_max, k=k, want_count=True)
        torch.cuda.synchronize()
    finally:
        for name, v in RESET.items():
            engine.set_option(name, v)
    return idx.cpu().numpy(), sc.cpu().numpy(), int(cnt.item())


def _run_all_paths(engine, e, p, rp_max, P):
    """{path: (idx, score, n_rescanned)} for every path the shape supports, each run twice (the runs must be bit-identical)."""
    out = {}
    paths = [(name, opts, 1) for name, opts in K1_PATHS] + [(f"gen{k}", {}, k) for k in (2, 3, 4) if k <= P]
    for name, opts, k in paths:
        a = _call(engine, e, p, rp_max, k, opts)
        b = _call(engine, e, p, rp_max, k, opts)
        assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1])), f"{name}: two runs of the same call differ"
        out[name] = a
    return out


def _compare(tag, out, ref_idx, ref_sc):
    bad = []
    for name, (idx, sc, cnt) in out.items():
        k = idx.shape[1]
        mi = int((idx != ref_idx[:, :k]).sum())
        ms = int((_bits(sc) != _bits(ref_sc[:, :k])).sum())
        print(f"{tag} path {name:5s} k={k} n_rescanned={cnt:6d} index mismatches={mi} score-bit mismatches={ms}")
        if mi or ms:
            rows = np.argwhere((idx != ref_idx[:, :k]) | (_bits(sc) != _bits(ref_sc[:, :k])))[:4]
            bad.append((name, mi, ms, [(int(n), int(q), int(idx[n, q]), int(ref_idx[n, q]), float(sc[n, q]), float(ref_sc[n, q])) for n, q in rows]))
    assert not bad, f"{tag}: (path, index mismatches, score-bit mismatches, first (row, slot, got, want, got score, want score)) = {bad}"


@pytest.mark.parametrize("kind,N,P,seed", FIXTURES, ids=[f"{k}-{N}x{P}-s{s}" for k, N, P, s in FIXTURES])
def test_every_path_equals_the_restatement_bit_for_bit(engine, kind, N, P, seed):
    E, Pm, info = R.KINDS[kind](N, P, seed)
    e, p = _norm(engine, E), _norm(engine, Pm)
    torch.cuda.synchronize()
    En, Pn = e[0].cpu().numpy(), p[0].cpu().numpy()
    kmax = min(4, P)
    ref_idx, ref_sc = R.topk(En, Pn, kmax)                 # once per fixture: the k best are a prefix of the kmax best (a total order)
    out = _run_all_paths(engine, e, p, p[2].max().reshape(1), P)
    tag = f"{kind} {N}x{P}"
    if N >= 65536:
        plan = (np.zeros(6, np.int32))
        lib, cu = sub("_lib").load_library(), sub("_lib").device_info(0)["compute_units"]
        assert lib.sdk_affinity_block_plan(N, P, cu, 1, plan.ctypes.data) == 0
        print(f"{tag}: block plan on {cu} compute units: taken={plan[0]} q={plan[1]} stages={plan[3]} parts={plan[4]} leftover items={plan[5]}")
        assert plan[0] == 1 and plan[3] >= 6, "this shape was chosen to HAVE a block plan with room for 3 records per sweep"
    _compare(tag, out, ref_idx, ref_sc)
    # the first column of every k > 1 equals every k = 1 path (implied by the parity above; stated because scoring_exact.hpp points here)
    for name, _ in K1_PATHS:
        for k in (2, 3, 4):
            if k <= P:
                assert np.array_equal(out[f"gen{k}"][0][:, 0], out[name][0][:, 0]) and np.array_equal(_bits(out[f"gen{k}"][1][:, 0]), _bits(out[name][1][:, 0]))
    # the fixture's own condition, on the device's result
    for name, (idx, sc, cnt) in out.items():
        R.check_fixture(kind, info, En, Pn, idx, sc, idx.shape[1])
    if kind == "knots":
        # planted rows sit in a knot of 16 profiles the bf16 coarse pass cannot separate, with 8 candidate slots: they must take the exact rescan
        # (the ratio of test_affinity_near_duplicates_force_rescan: 30 of 40).  At P > 32768 this is what proves the multi-slice rescan and the
        # merge's second pass ran; on the k = 1 fast path with N = 1 it is ONE flagged row: a partial quad (min(q * RS_ROWS + x, count - 1)).
        need = 0.75 * info["planted"]
        for name, (idx, sc, cnt) in out.items():
            assert cnt >= need, f"{tag} path {name}: {cnt} rows rescanned, {info['planted']} planted"
        if P > 32768:
            assert any((ko >= 32768).any() for ko in info["knot_of"])


def test_first_column_equals_every_k1_path(engine):
    """The claim of csrc/scoring_exact.hpp on its own, on a shape where all mechanisms differ: k = 1 on the fast path's plans and on the general
    depth-3 kernel, k = 2 on depth 3, k = 3 / 4 on depth 4 - one first column, bit for bit."""
    E, Pm, _ = R.knots(513, 1025, 3)
    e, p = _norm(engine, E), _norm(engine, Pm)
    out = _run_all_paths(engine, e, p, p[2].max().reshape(1), 1025)
    first = {name: (o[0][:, 0], _bits(o[1][:, 0])) for name, o in out.items()}
    for name, (i, s) in first.items():
        assert np.array_equal(i, first["fast"][0]) and np.array_equal(s, first["fast"][1]), name


NAN_SHAPES = [(33, 65), (129, 2049), (32, 32769)]


@pytest.mark.parametrize("N,P", NAN_SHAPES)
@pytest.mark.parametrize("rp", ["max", "nanmax"])
def test_nan_rows_follow_the_contract_on_every_path(engine, N, P, rp):
    """include/sdk_hip.h: a NaN score is never taken; a slot with no comparable score holds (-1, -inf) - never the kernels' internal 0x7fffffff.
    So a segment row with a NaN reports (-1, -inf) in every slot (backend.aggregate_matches skips a row < 0), a NaN profile row never wins, every
    other row stays bit-equal to the restatement, on every path, and the engine is fine afterwards.  `rp`: the caller's max profile residual is
    NaN (torch's max, what backend.py passes) or the finite max (nanmax); a NaN residual certifies nothing - every row takes the rescan.

    No path turns a non-finite score into an out-of-range read (read before this test was first run):
      general coarse   packed NaNs never enter the lists (v_max / v_med3 return the other operands; merge_chunk's `v > gv[q]` is false);
      general rescore  `if (ci[c] >= P) ci[c] = -1` and `ci[c] >= 0 && ci[c] < P` in front of the only indexed profile read;
      general rescan   profile rows `pp < p1 ? pp : p1 - 1`, inserts under `pp < p1`; segment rows come from flag_rows (row < N by construction);
      general merge    reads part_s / part_i under `ea < nsl * 4`, indexes nothing by a score;
      fast rescore     `if (pidx < P) first = pidx`, `bi >= 0 ? bi : 0`, `pidx < P && pidx != c_first`; the list is written under `m == M`, m < MAXC;
      fast rescan      `min(p0 + g, s1 - 1)`, `min(p0 + g + 32, s1 - 1)`, flagged rows `min(q * RS_ROWS + x, count - 1)`; the decoded key is stored only.
    The fast path's file is built -fno-honor-nans, so its NaN tests are on the bits (nan_bits)."""
    E, Pm, _ = R.gauss(N, P, 9)
    nan_row, nan_prof = min(3, N - 1), min(7, P - 1)
    E[min(5, N - 1)] = Pm[nan_prof] + np.float32(0.05) * E[0]          # a row whose best profile is the one that turns NaN
    E[nan_row, 10] = np.nan
    Pm[nan_prof, 100] = np.nan
    e, p = _norm(engine, E), _norm(engine, Pm)
    torch.cuda.synchronize()
    En, Pn = e[0].cpu().numpy(), p[0].cpu().numpy()
    assert np.isnan(En[nan_row]).any() and np.isnan(Pn[nan_prof]).any() and np.isfinite(np.delete(En, nan_row, 0)).all()
    rp_max = p[2].max().reshape(1) if rp == "max" else torch.nan_to_num(p[2], nan=0.0).max().reshape(1)
    assert bool(torch.isnan(rp_max).item()) == (rp == "max")
    ref_idx, ref_sc = R.topk(En, Pn, min(4, P))
    assert (ref_idx[nan_row] == -1).all() and not (ref_idx == nan_prof).any()
    out = _run_all_paths(engine, e, p, rp_max, P)
    for name, (idx, sc, cnt) in out.items():
        assert ((idx >= -1) & (idx < P)).all(), f"{name}: index outside [-1, P)"
        assert (idx[nan_row] == -1).all() and np.isneginf(sc[nan_row]).all(), f"{name}: the NaN row reports {idx[nan_row]}, {sc[nan_row]}"
        assert not (idx == nan_prof).any(), f"{name}: the NaN profile row won"
    _compare(f"nan[{rp}] {N}x{P}", out, ref_idx, ref_sc)
    # the next call on the engine is fine
    E2, P2, _ = R.gauss(33, 65, 10)
    e2, p2 = _norm(engine, E2), _norm(engine, P2)
    out2 = _run_all_paths(engine, e2, p2, p2[2].max().reshape(1), 65)
    ri, rs = R.topk(e2[0].cpu().numpy(), p2[0].cpu().numpy(), 4)
    _compare("after-nan 33x65", out2, ri, rs)


# ---- sdk_l2norm at its edges ---------------------------------------------------------------------------------------------------------------
def _bf16_rne(x):
    """fp32 -> bf16 (round to nearest even) -> fp32, on the bits."""
    b = _bits(np.asarray(x, dtype=np.float32)).astype(np.uint64)
    r = ((b + 0x7fff + ((b >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def _l2norm_in_order_fp32(X):
    """fp32 emulation of the kernel's sums in the kernel's order: lane l adds x[l]^2, x[l + 64]^2, ... (product rounded, then added), the 64
    partials meet in the xor tree 32, 16, .. 1; inv = 1 / max(sqrt(ss), 1e-12); e = x * inv."""
    X = np.asarray(X, dtype=np.float32)
    N, d = X.shape
    part = np.zeros((N, 64), dtype=np.float32)
    for c in range(0, d, 64):
        sq = (X[:, c:c + 64] * X[:, c:c + 64]).astype(np.float32)
        part[:, :sq.shape[1]] = (part[:, :sq.shape[1]] + sq).astype(np.float32)
    o = 32
    while o:
        part = (part + part[:, np.arange(64) ^ o]).astype(np.float32)
        o >>= 1
    ss = part[:, :1]
    inv = (np.float32(1.0) / np.maximum(np.sqrt(ss, dtype=np.float32), np.float32(1e-12))).astype(np.float32)
    return (X * inv).astype(np.float32)


def _l2norm_rows(N, d, seed):
    """Gaussian times 7, and - as far as N allows, in this order - a zero row, a row whose single non-zero element is +-1, a row of norm 1e18
    (its square sum 1e36 is finite in fp32), a row of norm 1e-14 (below the 1e-12 floor)."""
    rng = np.random.default_rng([seed, N, d])
    X = (rng.standard_normal((N, d)) * 7).astype(np.float32)
    kinds = {}
    special = ["zero", "one", "huge", "tiny"]
    if N == 1:
        special = [special[seed % 4]]
    for i, what in enumerate(special[:N]):
        r = (N - 1 - i) if N > 1 else 0                   # from the END: the last, partly filled block of four rows holds edge rows
        kinds[r] = what
        if what == "zero":
            X[r] = 0
        elif what == "one":
            X[r] = 0
            X[r, (7 * d) // 8 + 1] = -1.0 if seed % 2 else 1.0
        elif what == "huge":
            X[r] = R.l2n(X[r][None])[0] * np.float32(1e18)
        else:
            X[r] = R.l2n(X[r][None])[0] * np.float32(1e-14)
    return X, kinds


@pytest.mark.parametrize("d", [64, 192, 256, 512])
@pytest.mark.parametrize("N", [1, 3, 4, 5, 257])
def test_l2norm_edges(engine, N, d):
    """Four rows per block (N = 1, 3, 4, 5, 257), one to eight elements per lane (d = 64 .. 512), and the rows the floor, the range and exact
    representability single out.
      Eb    == RNE bf16 of the device's own E, bit for bit.
      resid >= (1 - 1e-4) |E - Eb| (float64, from the device's E and Eb): the affinity certificate multiplies resid by 1.0001 and has no other
               slack for it, so UNDERSTATING is the unsound direction; above, the existing rtol 1e-4 (atol 1e-9).
      E     against float64 x / max(|x|, 1e-12), per row: the yardstick is the distance from float64 of an in-order fp32 emulation of the
               kernel's own sums; bound = 4 x yardstick + 1 fp32 ulp of the row's largest element (the margin covers `ss += x * x` contracted
               into an fma or not, and the rounding of the division and the square root); at d = 192 the existing atol of 2e-7 as well."""
    for seed in range(4 if N == 1 else 1):
        X, kinds = _l2norm_rows(N, d, seed)
        E, Eb, r = _norm(engine, X)
        torch.cuda.synchronize()
        E, Ebf, r = E.cpu().numpy(), Eb.float().cpu().numpy(), r.cpu().numpy()
        assert np.isfinite(E).all() and np.isfinite(r).all()
        assert np.array_equal(_bits(Ebf), _bits(_bf16_rne(E))), "Eb is not the RNE bf16 rounding of E"
        rr = np.sqrt(((E.astype(np.float64) - Ebf.astype(np.float64)) ** 2).sum(1))
        low = float((r.astype(np.float64) / np.where(rr > 0, rr, 1.0))[rr > 0].min()) if (rr > 0).any() else 1.0
        assert (r.astype(np.float64) >= (1 - 1e-4) * rr).all(), f"resid understated: min ratio {low}"
        assert np.allclose(r.astype(np.float64), rr, rtol=1e-4, atol=1e-9)
        x64 = X.astype(np.float64)
        ref = x64 / np.maximum(np.sqrt((x64 ** 2).sum(1, keepdims=True)), 1e-12)
        yard = np.abs(_l2norm_in_order_fp32(X).astype(np.float64) - ref).max(1)
        bound = 4 * yard + np.spacing(np.abs(ref).max(1).astype(np.float32)).astype(np.float64)
        err = np.abs(E.astype(np.float64) - ref).max(1)
        worst = int(np.argmax(err / bound))
        print(f"l2norm N={N} d={d} seed={seed}: max err {err.max():.3e}, yardstick {yard.max():.3e}, worst err/bound {err[worst] / bound[worst]:.3f} (row {worst}), "
              f"min resid / |E - Eb| {low:.7f}")
        assert (err <= bound).all(), (worst, err[worst], bound[worst], kinds.get(worst))
        if d == 192:
            assert err.max() <= 2e-7
        for row, what in kinds.items():
            if what == "zero":
                assert not E[row].any() and not Ebf[row].any() and r[row] == 0
            elif what == "one":                         # exactly representable: E exact, Eb exact, residual exactly 0
                assert np.array_equal(E[row], X[row]) and np.array_equal(Ebf[row], X[row]) and r[row] == 0
            elif what == "tiny":                        # below the floor: scaled by 1 / 1e-12, not to unit norm
                assert abs(float(np.sqrt((E[row].astype(np.float64) ** 2).sum())) - 1e-2) < 1e-6
            else:
                assert abs(float(np.sqrt((E[row].astype(np.float64) ** 2).sum())) - 1.0) < 1e-6
