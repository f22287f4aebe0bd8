"""Host restatement of the exact pass of sdk_affinity_topk (csrc/scoring_exact.hpp), numpy only, for BIT-FOR-BIT comparison.

The device scores a (segment, profile) pair with one routine, whatever kernel calls it: lane j of 8 owns the elements 32 q + 4 j + 0..3,
q = 0..5, and runs 24 sequential fp32 fused multiply-adds over them (q ascending, then the element), starting from +0; the eight lane sums meet in
the xor butterfly 1, 2, 4, i.e. ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)) in fp32.  Explicit fmaf and plain adds leave the compiler
nothing to contract or reorder, so a host that repeats the order with a CORRECTLY ROUNDED fma reproduces every score bit.

fma32 is that fma: the product of two fp32 values is exact in float64 (48 bits), the addend joins it through TwoSum, the float64 sum is rounded
TO ODD with the residual as the sticky bit, and 53 - 24 >= 2 spare bits make the final RNE conversion to fp32 the single rounding of the exact
a * b + c.  (float32(float64(a) * float64(b) + float64(c)) rounds twice and is wrong on ties: tests/test_affinity_ref_cpu.py shows cases.)

topk returns what the header promises: the k best by better() - higher score first, then the LOWER index - of the fp32 full scan, and the NaN
contract of include/sdk_hip.h: a NaN score is never taken, a slot without a comparable score holds (-1, -inf).
"""
from __future__ import annotations

import numpy as np

D = 192
U32 = 2.0 ** -24                                   # fp32 unit roundoff
GAMMA27 = 27 * U32 / (1 - 27 * U32)                # 24 sequential fma + 3 levels of adds (test_affinity_ref_cpu.py derives the bound)

# element owned by lane j at step s = 4 q + t: 32 q + 4 j + t
_STEP_IDX = np.array([[32 * (s // 4) + 4 * j + (s % 4) for j in range(8)] for s in range(24)])      # [24][8]


def fma32(a, b, c):
    """Correctly rounded fp32 a * b + c, element-wise (finite operands whose product and sum stay inside float64's normal range)."""
    a64, b64, c64 = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    p = a64 * b64                                  # exact: 24 x 24 bits
    s = p + c64
    bb = s - p                                     # TwoSum (Knuth): s + err == p + c exactly
    err = (p - (s - bb)) + (c64 - bb)
    s = np.ascontiguousarray(s)
    bits = s.view(np.int64)
    # round to odd: the sum is inexact and RN landed on an even mantissa -> the other neighbour of the exact value (the one on err's side) is the
    # odd one.  In sign-magnitude bits "away from zero" is +1.
    fix = (err != 0) & ((bits & 1) == 0)
    away = (err > 0) == (s > 0)
    bits = bits + np.where(fix, np.where(away, 1, -1), 0)
    with np.errstate(invalid="ignore", over="ignore"):
        return bits.view(np.float64).astype(np.float32)


def fma32_naive(a, b, c):
    """The float64-rounded-once emulation: TWO roundings (float64, then fp32).  Kept to show the difference."""
    a64, b64, c64 = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    return (a64 * b64 + c64).astype(np.float32)


def _combine(acc):
    """fp32 xor butterfly 1, 2, 4 over the last axis (8 lanes)."""
    a = acc.astype(np.float32)
    s1 = a[..., 0::2] + a[..., 1::2]               # (a0+a1) (a2+a3) (a4+a5) (a6+a7)
    s2 = s1[..., 0::2] + s1[..., 1::2]
    return (s2[..., 0] + s2[..., 1]).astype(np.float32)


def dot192_pairs(E, P):
    """Score of row i of E with row i of P, the device's arithmetic: [n] fp32."""
    E = np.asarray(E, dtype=np.float32)
    P = np.asarray(P, dtype=np.float32)
    assert E.shape == P.shape and E.shape[-1] == D
    out = np.empty(E.shape[0], dtype=np.float32)
    for lo in range(0, E.shape[0], 1 << 16):
        e, p = E[lo:lo + (1 << 16)], P[lo:lo + (1 << 16)]
        acc = np.zeros((e.shape[0], 8), dtype=np.float32)
        for s in range(24):
            acc = fma32(e[:, _STEP_IDX[s]], p[:, _STEP_IDX[s]], acc)
        out[lo:lo + e.shape[0]] = _combine(acc)
    return out


def dot192(E, P, block: int = 2048):
    """The full [N][Pn] fp32 score matrix in the device's arithmetic, in blocks of profiles (N * block * 8 float64 live at a time)."""
    E = np.asarray(E, dtype=np.float32)
    P = np.asarray(P, dtype=np.float32)
    N, Pn = E.shape[0], P.shape[0]
    out = np.empty((N, Pn), dtype=np.float32)
    blk = max(1, min(block, (1 << 18) // max(1, N)))
    for lo in range(0, Pn, blk):
        p = P[lo:lo + blk]
        acc = np.zeros((N, p.shape[0], 8), dtype=np.float32)
        for s in range(24):
            acc = fma32(E[:, None, _STEP_IDX[s]], p[None, :, _STEP_IDX[s]], acc)
        out[:, lo:lo + p.shape[0]] = _combine(acc)
    return out


def scan64(E, P):
    """The float64 scan [N][Pn]."""
    with np.errstate(invalid="ignore"):
        return np.asarray(E, dtype=np.float64) @ np.asarray(P, dtype=np.float64).T


def better(s, i, s2, i2):
    return s > s2 or (s == s2 and i < i2)


def topk_of_scores(S, k):
    """The k best of every row of an fp32 score matrix by better(); NaN never taken; empty slots (-1, -inf)."""
    N, Pn = S.shape
    if k > Pn:
        raise ValueError("k > P")
    key = np.where(np.isnan(S), -np.inf, S).astype(np.float32)       # (finite unit rows never score -inf, so a NaN sorts behind every score)
    order = np.lexsort((np.broadcast_to(np.arange(Pn), S.shape), -key.astype(np.float64)), axis=1)[:, :k]      # score desc, index asc
    idx = order.astype(np.int32)
    sc = np.take_along_axis(S, order, 1).astype(np.float32)
    empty = np.isnan(sc)
    idx[empty] = -1
    sc[empty] = -np.inf
    return idx, sc


def topk(E, P, k, full: bool = False):
    """(idx [N][k] int32, score [N][k] fp32) of the fp32 full scan in the device's arithmetic.

    full = False scores exactly only the pairs that can be among the k best, found with the float64 scan: |dot192 - scan64| <= B :=
    GAMMA27 * max|e| * max|p| + 1e-12 (derived in tests/test_affinity_ref_cpu.py), k profiles have scan64 >= v_k (the k-th best scan64 score of
    the row), hence fp32 score >= v_k - B, and a profile with scan64 < v_k - 2 B has fp32 score < v_k - B: at least k others beat it strictly.
    full = True scores everything (the CPU test compares the two)."""
    E = np.asarray(E, dtype=np.float32)
    P = np.asarray(P, dtype=np.float32)
    N, Pn = E.shape[0], P.shape[0]
    assert 1 <= k <= Pn
    if full:
        return topk_of_scores(dot192(E, P), k)
    ne = np.sqrt((np.nan_to_num(E).astype(np.float64) ** 2).sum(1)).max()
    npn = np.sqrt((np.nan_to_num(P).astype(np.float64) ** 2).sum(1)).max()
    B = GAMMA27 * ne * npn + 1e-12
    idx = np.full((N, k), -1, dtype=np.int32)
    sc = np.full((N, k), -np.inf, dtype=np.float32)
    step = max(1, (1 << 22) // Pn)                                          # rows per pass: the float64 scan stays at 32 MB
    for lo in range(0, N, step):
        S64 = scan64(E[lo:lo + step], P)
        nan = np.isnan(S64)
        key = np.where(nan, -np.inf, S64)
        vk = -np.partition(-key, k - 1, axis=1)[:, k - 1]                   # k-th best (a row with fewer than k comparable scores: -inf, all stay)
        rows, cols = np.nonzero((key >= (vk - 2 * B)[:, None]) & ~nan)
        if not rows.size:
            continue
        s = dot192_pairs(E[lo + rows], P[cols])
        o = np.lexsort((cols, -s.astype(np.float64), rows))                 # per row: score desc, index asc
        rows, cols, s = rows[o], cols[o], s[o]
        rank = np.arange(rows.size) - np.searchsorted(rows, rows)           # position inside the row's run
        keep = rank < k
        idx[lo + rows[keep], rank[keep]] = cols[keep]
        sc[lo + rows[keep], rank[keep]] = s[keep]
    return idx, sc


# ---- fixtures (seeded; RAW fp32 rows: the device normalises them, the CPU test uses l2n below) -----------------------------------------------
def l2n(x):
    """Row-wise x / max(|x|, 1e-12), norm in float64, result fp32 (the CPU stand-in for sdk_l2norm)."""
    x = np.asarray(x, dtype=np.float32)
    n = np.sqrt((x.astype(np.float64) ** 2).sum(-1, keepdims=True))
    return (x / np.maximum(n, 1e-12)).astype(np.float32)


def _g(rng, n):
    return l2n(rng.standard_normal((n, D)).astype(np.float32))


BORDERS = (32, 1024, 2048, 32768)      # first index of a tile / of an index chunk and rescan slice / past the depth-3 range / of the 33rd slice
KNOT = 16                              # near-copies per direction: more than the 8 candidate slots


def gauss(N, P, seed):
    rng = np.random.default_rng([seed, N, P, 1])
    return _g(rng, N), _g(rng, P), {}


def knots(N, P, seed):
    """16 near-copies (noise 1e-4 .. 3e-4, below bf16 resolution) of each of up to 4 directions; the LAST knot ends at index P - 1 (for
    P > 32768: inside the last rescan slice), the others start at multiples of 1024 minus 8 where they fit, so they straddle a chunk border.
    Planted segment rows sit next to a direction: info['planted'] rows, info['knot_of'] their knot's profile indices."""
    rng = np.random.default_rng([seed, N, P, 2])
    Pm = _g(rng, P)
    nk = max(1, min(4, P // KNOT))
    size = min(KNOT, P)
    starts = [P - size] + [s for s in (1016, 2040, 24) if s + size <= P - size][: nk - 1]
    dirs = _g(rng, len(starts))
    for d, s0 in zip(dirs, starts):
        sig = rng.uniform(1e-4, 3e-4, (size, 1)).astype(np.float32)
        Pm[s0:s0 + size] = d[None] + sig * _g(rng, size)
    E = _g(rng, N)
    # planted rows: a count that is no multiple of 4 (the k = 1 rescan works on quads of flagged rows; the last quad is then partial)
    npl = N if N < 4 else min(N - (1 if N % 4 == 0 else 0), 41)
    npl -= 1 if (npl % 4 == 0 and npl > 1) else 0
    which = np.arange(npl) % len(starts)
    E[:npl] = dirs[which] + np.float32(0.05) * _g(rng, npl)
    return E, Pm, {"planted": npl, "knot_of": [np.arange(starts[w], starts[w] + size) for w in which]}


def dups(N, P, seed):
    """Profile b is an exact copy of profile b - 1 for every border b < P; row i of the first rows sits next to pair i."""
    rng = np.random.default_rng([seed, N, P, 3])
    Pm = _g(rng, P)
    E = _g(rng, N)
    pairs = [b for b in BORDERS if b < P]
    for b in pairs:
        Pm[b] = Pm[b - 1]
    rows = {}
    for i, b in enumerate(pairs[:N] if N >= len(pairs) else pairs[-N:]):
        E[i] = Pm[b] + np.float32(0.05) * _g(rng, 1)[0]
        rows[i] = b
    return E, Pm, {"dup_rows": rows}


def ends(N, P, seed):
    """Even rows (the first 8) sit next to profile 0, odd rows next to profile P - 1."""
    rng = np.random.default_rng([seed, N, P, 4])
    Pm = _g(rng, P)
    E = _g(rng, N)
    rows = {}
    for i in range(min(N, 8)):
        t = 0 if (i + seed) % 2 == 0 else P - 1
        E[i] = Pm[t] + np.float32(0.05) * _g(rng, 1)[0]
        rows[i] = t
    return E, Pm, {"end_rows": rows}


def negative(N, P, seed):
    """Every profile in the half-space opposite every segment: all scores < 0."""
    rng = np.random.default_rng([seed, N, P, 5])
    v = _g(rng, 1)[0]
    E = v[None] + np.float32(0.3) * _g(rng, N)
    Pm = -v[None] + np.float32(0.3) * _g(rng, P)
    return E.astype(np.float32), Pm.astype(np.float32), {}


def zeros(N, P, seed):
    """negative() with an all-zero profile row (it must win every non-zero segment with score 0) and, for N > 1, an all-zero segment row
    (every score +0.0: indices 0 .. k - 1).  N = 1: the zero SEGMENT row on even seeds, the zero profile alone on odd ones."""
    E, Pm, _ = negative(N, P, seed)
    zp = (P - 1) if seed % 2 else P // 2
    zrow = None
    if N > 1 or seed % 2 == 0:
        zrow = N // 2
        E[zrow] = 0
    Pm[zp] = 0
    return E, Pm, {"zero_profile": zp, "zero_row": zrow}


KINDS = {"gauss": gauss, "knots": knots, "dups": dups, "ends": ends, "negative": negative, "zeros": zeros}


def check_fixture(kind, info, En, Pn, idx, sc, k):
    """The fixture's own condition on a top-k result (the restatement's on the CPU, the device's on the GPU).  En, Pn are the normalised rows."""
    N, P = En.shape[0], Pn.shape[0]
    if kind == "knots":
        S = scan64(En[:info["planted"]], Pn)
        for n in range(info["planted"]):
            close = int((S[n] >= S[n].max() - 1e-3).sum())
            assert close >= min(12, P), f"knots: planted row {n} has only {close} profiles within 1e-3 of its best: the certificate could settle it"
            assert idx[n, 0] in info["knot_of"][n], (n, idx[n])
    elif kind == "dups":
        for n, b in info["dup_rows"].items():
            assert idx[n, 0] == b - 1, f"dups: row {n} next to the pair ({b - 1}, {b}) reports {idx[n]}"
            if k >= 2:
                assert idx[n, 1] == b and sc[n, 0].view(np.uint32) == sc[n, 1].view(np.uint32), (n, idx[n], sc[n])
    elif kind == "ends":
        for n, t in info["end_rows"].items():
            assert idx[n, 0] == t, f"ends: row {n} next to profile {t} reports {idx[n]}"
    elif kind == "negative":
        assert (sc < 0).all() and (scan64(En, Pn) < -0.1).all()
    elif kind == "zeros":
        zp, zr = info["zero_profile"], info["zero_row"]
        for n in range(N):
            if n == zr:
                assert list(idx[n]) == list(range(k)) and (sc[n].view(np.uint32) == 0).all(), f"zeros: the zero segment row reports {idx[n]}, {sc[n]}"
            else:
                assert idx[n, 0] == zp and sc[n, 0].view(np.uint32) == 0, f"zeros: row {n} reports {idx[n]}, {sc[n]} (zero profile {zp})"
                assert (sc[n, 1:] < 0).all()
