"""Fusing several diarizations of one recording into one: label mapping and weighted voting in the manner of DOVER-Lap, computed on the
device for a pack of recordings (Backend.fuse_diarizations / compare_diarizations / diarize_fused).  The rule below is THIS build's
statement; it follows the method as published (labels mapped through pairwise co-occurrence starting from the hypothesis that agrees most
with the others, hypotheses ranked by mean disagreement and weighted by rank, a per-frame vote with the speaker count taken from the
weighted mean), but no code of DOVER or DOVER-Lap is on hand, so PARITY IS UNPINNED and the tests pin this rule.  Every quantity is an
integer and every tie has a stated winner: host and device agree bit for bit.

  inputs      R recordings, each with the same number H of hypotheses, 2 <= H <= MAX_FUSE_HYPS = 8.  Hypothesis h of recording r has
              K[h][r] <= 64 speakers and a mask m_h[g] (uint64) per frame of the recording's G_r frames on the global grid of score.py
              (frame g has centre sample 270 g + 495): bit k is set iff speaker k is active.  Bits at or above K[h][r] name nobody and are
              ignored everywhere (K = 64 works: the valid bits are never built as (1 << K) - 1 in 64-bit arithmetic).  A mask may have any
              number of bits set.  All hypotheses of a recording share G_r
  forms       a hypothesis is a DiarizationResult (any object with speakers [G, 2] and n_speakers): bit k is set iff speakers[g] names k
              with 0 <= k < K; an entry below 0 or at or above K names nobody and a name twice counts once.  Or a turn list [(start_s,
              end_s, name)]: it goes through score.prepare_reference and sdk_score_reference with no collar and no overlap skipping;
              speaker i is the i-th name in that function's numbering
  tables      with h-major groups (h, r), spk_off [H R + 1] int32 = the prefix sums of K[h][r]; the masks are [H][G] uint64 on the packed
              grid with frame_off [R + 1].  Pairs (a, b), a < b, are numbered lexicographically, p = a (2 H - a - 1) / 2 + (b - a - 1),
              P = H (H - 1) / 2 <= 28; the pair groups are q = p R + r.  row_off, col_off [P R + 1] int32 = the prefix sums of K[a][r] and
              K[b][r], co_off [P R + 1] int64 those of their products: exactly the ref_off, cent_off and co_off sdk_score_map takes, with
              P R "recordings"
  1 pairs     for every q, co_q [K_a][K_b] int32 = the frames in which bit i of m_a and bit j of m_b are both set; tally_q [2] int64 =
              (sum_g max(n_a, n_b), sum_g min(n_a, n_b)), n = the number of valid bits.  sdk_score_map then runs once on these tables as
              they stand and gives correct_q, the value of the exact maximum-weight assignment: unique even where the map is not
  2 rank      dis[a][b] = dis[b][a] = sum max - correct (the symmetric DER numerator: count differences plus confusion); D_h = the sum
              of dis[h][b] over b != h; order = the hypotheses by ascending D_h, ties to the lower h.  w_h = the caller's weight with
              weights= (H integers in 1 .. 65536, the same for every recording), else FUSE_RANK_WEIGHTS[rank of h], DOVER-Lap's rank
              weighting floor(65536 (k + 1)^-0.1) written out below as eight literals that the device is handed as a table (no pow runs
              where host and device could differ)
  3 labels    fused labels are numbered per recording, at most 64.  The anchor order[0] keeps its own numbers: label_of[anchor][i] = i, L =
              K_anchor.  For k = 1 .. H - 1, h = order[k]: A[u][j] (int64, u < L, j < K_h) = the sum, over the earlier hypotheses h' and
              their speakers i with label_of[h'][i] == u, of co(h', h)[i][j] - the unweighted frame count, the pair's table read transposed
              when h' > h.  Greedily: repeatedly the largest A[u][j] > 0 among unused u and unmapped j, the lowest u and then the lowest j
              on ties, sets label_of[h][j] = u, until none is positive.  The unmapped j in ascending order: while L < 64, label_of[h][j] =
              L++; otherwise label_of[h][j] = -1 and the recording's overflow counts one more.  Two speakers of one hypothesis never share
              a label.  Greedy and not the exact assignment: the voted output depends on the map itself, and only greedy with stated ties
              makes the map unique
  4 vote      for frame g: c_h = the number of valid bits of m_h[g] (mapped or not), seen_h = the set of labels >= 0 of those bits, v[u] =
              the sum of w_h over the h with u in seen_h, W = the sum of the w_h, n = min(cap, floor((2 sum_h w_h c_h + W) / (2 W))) - the
              weighted mean count, halves rounded up; cap = diarize_host._speaker_cap(max_speakers), 1 or 2, as in smooth.py.  The output
              frame names the labels with v > 0 that come first in the order (v descending, u ascending), at most n of them, in that order
              from slot 0; empty slots hold -1.  Labels keep their numbers: a label that wins no frame has no turn
  5 tallies   per recording [4] int64: speech = the frames that name somebody, overlap = the frames that name two, unanimous = the frames in
              which the H sets seen_h are all equal (the all-empty frames included), overflow = the count of step 3

The device path (csrc/fuse.hip) is four calls with sdk_score_map between the second and the third, in stream order: sdk_fuse_masks (one
thread per frame, once per hypothesis), sdk_fuse_cooccur (all P pairs in one launch; a workgroup takes FUSE_BLOCK_FRAMES = 256 packed frames
of one pair and sums its [64][64] int32 table in LDS, then one integer atomic per non-zero cell), sdk_score_map, sdk_fuse_labels (one wave
per recording: steps 2 and 3, A in LDS, the arg-max of a greedy step a wave reduction) and sdk_fuse_vote (one thread per frame: steps 4 and
5, a running best two over the set bits of the union of the seen_h).  No call takes a workspace, nothing waits for the device, and a pack
costs one upload and one download.  fuse_host restates the rule in numpy; it calls score.assignment_host for `correct`.
"""
from __future__ import annotations

import copy
import numbers
from dataclasses import dataclass
from typing import TYPE_CHECKING, List, Optional, Sequence

import numpy as np

from .diarize_host import _speaker_cap, global_frames, turns_from_frames
from .score import MAX_SCORE_SPEAKERS, assignment_host, prepare_reference

if TYPE_CHECKING:
    from .backend import Backend

MAX_FUSE_HYPS = 8                # FUSE_MAX_HYPS of csrc/fuse.hip
MAX_FUSE_SPEAKERS = MAX_SCORE_SPEAKERS   # speakers of a hypothesis, and fused labels of a recording (PG_MAX_SPK)
FUSE_BLOCK_FRAMES = 256          # the packed frames one workgroup of sdk_fuse_cooccur and sdk_fuse_vote serves (FUSE_NT)
MAX_FUSE_WEIGHT = 65536
FUSE_RANK_WEIGHTS = (65536, 61147, 58717, 57052, 55793, 54785, 53947, 53231)   # floor(65536 (k + 1) ** -0.1), k = 0 .. 7 ("2 rank")


# ------------------------------------------------------------------------------------------------ tables
def pairs(H: int) -> list:
    """The pairs (a, b), a < b, in the order of their numbers p."""
    return [(a, b) for a in range(H) for b in range(a + 1, H)]


def pair_index(a: int, b: int, H: int) -> int:
    return a * (2 * H - a - 1) // 2 + (b - a - 1)


def _check_hyps(who: str, H: int) -> int:
    if not 2 <= int(H) <= MAX_FUSE_HYPS:
        raise ValueError(f"{who}: H={H} hypotheses per recording (2 .. {MAX_FUSE_HYPS})")
    return int(H)


def check_weights(who: str, weights, H: int) -> Optional[np.ndarray]:
    """weights=: None, or H integers in 1 .. 65536 -> None or [H] int32."""
    if weights is None:
        return None
    w = list(weights)
    if len(w) != H or any(isinstance(x, bool) or not isinstance(x, numbers.Integral) or not 1 <= x <= MAX_FUSE_WEIGHT for x in w):
        raise ValueError(f"{who}: weights={weights!r} (None, or H = {H} integers in 1 .. {MAX_FUSE_WEIGHT})")
    return np.asarray(w, dtype=np.int32)


def check_cap(who: str, cap) -> int:
    if isinstance(cap, bool) or cap not in (1, 2):
        raise ValueError(f"{who}: cap={cap!r} (1 or 2 speakers per frame)")
    return int(cap)


class FuseTables:
    """The prefix-sum tables of a pack ("tables" in the module docstring), on the host; to(eng) puts them on the device in one upload
    (frame_off_d, spk_off_d, row_off_d, col_off_d, co_off_d, rank_weight_d)."""

    def __init__(self, K, frame_off, who: str = "fuse"):
        K = np.asarray(K, dtype=np.int64)
        if K.ndim != 2:
            raise ValueError(f"{who}: K must be [H, R], got {list(K.shape)}")
        self.H, self.R = _check_hyps(who, K.shape[0]), int(K.shape[1])
        frame_off = np.asarray(frame_off, dtype=np.int64).reshape(-1)
        if self.R < 1 or frame_off.shape != (self.R + 1,) or frame_off[0] != 0 or (np.diff(frame_off) < 0).any():
            raise ValueError(f"{who}: frame_off must hold R + 1 = {self.R + 1} >= 2 prefix sums from 0, got {frame_off.tolist()[:8]}")
        if (K < 0).any() or (K > MAX_FUSE_SPEAKERS).any():
            raise ValueError(f"{who}: {int(K.max())} speakers in a hypothesis (0 .. {MAX_FUSE_SPEAKERS})")
        self.K, self.frame_off, self.G = K, frame_off, int(frame_off[-1])
        if self.G >= 1 << 30:
            raise ValueError(f"{who}: {self.G} frames in one pack (fewer than 2^30)")
        self.P = self.H * (self.H - 1) // 2
        self.max_spk = int(K.max()) if K.size else 0
        self.spk_off = np.concatenate([[0], np.cumsum(K.reshape(-1))]).astype(np.int64)
        Ka = np.concatenate([K[a] for a, _ in pairs(self.H)])
        Kb = np.concatenate([K[b] for _, b in pairs(self.H)])
        self.row_off = np.concatenate([[0], np.cumsum(Ka)]).astype(np.int64)
        self.col_off = np.concatenate([[0], np.cumsum(Kb)]).astype(np.int64)
        self.co_off = np.concatenate([[0], np.cumsum(Ka * Kb)]).astype(np.int64)
        self.n_spk, self.n_rows, self.co_total = int(self.spk_off[-1]), int(self.row_off[-1]), int(self.co_off[-1])
        self.frame_off_d = self.spk_off_d = self.row_off_d = self.col_off_d = self.co_off_d = self.rank_weight_d = None

    def host_parts(self) -> list:
        """The int32 pieces of the upload, co_off (int64, viewed as int32 pairs) first so that it stays 8-byte aligned."""
        return [self.co_off.astype("<i8").view(np.int32), self.frame_off.astype(np.int32), self.spk_off.astype(np.int32), self.row_off.astype(np.int32),
                self.col_off.astype(np.int32), np.asarray(FUSE_RANK_WEIGHTS, dtype=np.int32)]

    def bind(self, up) -> int:
        """up: the uploaded int32 tensor that starts with host_parts() -> the number of its elements these tables take."""
        import torch
        n = [2 * (self.P * self.R + 1), self.R + 1, self.H * self.R + 1, self.P * self.R + 1, self.P * self.R + 1, MAX_FUSE_HYPS]
        cut = np.cumsum([0] + n).tolist()
        self.co_off_d = up[cut[0]:cut[1]].view(torch.int64)
        self.frame_off_d, self.spk_off_d, self.row_off_d, self.col_off_d, self.rank_weight_d = (up[a:b] for a, b in zip(cut[1:-1], cut[2:]))
        return cut[-1]

    def to(self, eng) -> "FuseTables":
        import torch
        self.bind(torch.from_numpy(np.concatenate(self.host_parts())).to(eng.device))
        return self


# ------------------------------------------------------------------------------------------------ the rule on the host
def valid_bits(K: int) -> np.uint64:
    return np.uint64(0xFFFFFFFFFFFFFFFF) if K >= 64 else np.uint64((1 << max(int(K), 0)) - 1)


def masks_host(speakers, K: int) -> np.ndarray:
    """sdk_fuse_masks for one recording in numpy: speakers [G, 2], K speakers -> mask [G] uint64 ("forms" in the module docstring)."""
    sp = np.asarray(speakers, dtype=np.int64).reshape(-1, 2)
    m = np.zeros(sp.shape[0], np.uint64)
    for s in range(2):
        on = (sp[:, s] >= 0) & (sp[:, s] < min(int(K), 64))
        m[on] |= np.uint64(1) << sp[on, s].astype(np.uint64)
    return m


def turns_mask_host(turns, G: int):
    """A turn list on G frames -> (mask [G] uint64, names): score.prepare_reference, then the reference rasteriser without collar."""
    from .score import reference_masks_host
    merged, names = prepare_reference(turns)
    return reference_masks_host(merged, G)[0], names


def _active(mask, K: int) -> np.ndarray:
    """mask [G] uint64 -> [G, K] bool: speaker k is active (the bits at or above K are dropped)."""
    m = np.asarray(mask, dtype=np.uint64)
    return ((m[:, None] >> np.arange(K, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool).reshape(len(m), K)


def cooccur_host(ma, Ka: int, mb, Kb: int):
    """sdk_fuse_cooccur for one pair of one recording in numpy -> (co [Ka, Kb] int32, tally [2] int64 = (sum max, sum min))."""
    A, B = _active(ma, Ka), _active(mb, Kb)
    na, nb = A.sum(1).astype(np.int64), B.sum(1).astype(np.int64)
    co = np.rint(A.T.astype(np.float64) @ B.astype(np.float64)).astype(np.int32).reshape(Ka, Kb)      # counts below 2^30: exact in float64
    return co, np.array([np.maximum(na, nb).sum(), np.minimum(na, nb).sum()], np.int64)


def labels_host(co: dict, dis, K: Sequence[int], weights=None):
    """sdk_fuse_labels for one recording in numpy: co {(a, b): [K_a, K_b]} for a < b, dis [H, H], K [H] -> (order [H], weight [H], label_of
    (a list of H int32 arrays), n_labels, overflow): "2 rank" and "3 labels" in the module docstring."""
    H = len(K)
    D = np.asarray(dis, dtype=np.int64).sum(1)
    order = sorted(range(H), key=lambda h: (int(D[h]), h))
    weight = np.zeros(H, np.int32)
    for rank, h in enumerate(order):
        weight[h] = int(weights[h]) if weights is not None else FUSE_RANK_WEIGHTS[rank]
    label_of = [np.full(int(k), -1, np.int32) for k in K]
    label_of[order[0]][:] = np.arange(int(K[order[0]]))
    L, overflow = int(K[order[0]]), 0
    for k in range(1, H):
        h = order[k]
        A = np.zeros((L, int(K[h])), np.int64)
        for hp in order[:k]:
            t = np.asarray(co[(hp, h)], dtype=np.int64) if hp < h else np.asarray(co[(h, hp)], dtype=np.int64).T
            for i, u in enumerate(label_of[hp].tolist()):
                if u >= 0:
                    A[u] += t[i]
        while A.size and A.max() > 0:
            u, j = np.unravel_index(int(np.argmax(A)), A.shape)             # the first maximum in row-major order: the lowest u, then the lowest j
            label_of[h][j] = u
            A[u, :] = 0
            A[:, j] = 0
        for j in np.nonzero(label_of[h] < 0)[0].tolist():
            if L < MAX_FUSE_SPEAKERS:
                label_of[h][j], L = L, L + 1
            else:
                overflow += 1
    return np.asarray(order, np.int32), weight, label_of, L, overflow


def vote_host(masks, K: Sequence[int], label_of, weight, cap: int):
    """sdk_fuse_vote for one recording in numpy: masks [H][G] uint64 -> (speakers [G, 2] int32, (speech, overlap, unanimous))."""
    H, G = len(K), len(masks[0])
    seen = np.zeros((H, G, MAX_FUSE_SPEAKERS), bool)
    wc = np.zeros(G, np.int64)
    for h in range(H):
        on = _active(masks[h], int(K[h]))
        wc += int(weight[h]) * on.sum(1).astype(np.int64)
        for i, u in enumerate(np.asarray(label_of[h]).tolist()):
            if u >= 0:
                seen[h, :, u] |= on[:, i]
    W = int(np.asarray(weight, dtype=np.int64).sum())
    n = np.minimum(int(cap), (2 * wc + W) // (2 * W))
    v = np.zeros((G, MAX_FUSE_SPEAKERS), np.int64)
    for h in range(H):
        v += seen[h] * np.int64(weight[h])
    first = np.argsort(-v, axis=1, kind="stable")[:, :2]                    # v descending, u ascending
    out = np.full((G, 2), -1, np.int32)
    for s in range(2):
        ok = (np.take_along_axis(v, first[:, s:s + 1], 1)[:, 0] > 0) & (n > s)
        out[ok, s] = first[ok, s]
    unanimous = np.ones(G, bool)
    for h in range(1, H):
        unanimous &= (seen[h] == seen[0]).all(1)
    return out, (int((out[:, 0] >= 0).sum()), int((out[:, 1] >= 0).sum()), int(unanimous.sum()))


def fuse_host(masks, frame_off, K, weights=None, cap: int = 2) -> dict:
    """The whole rule for a pack in numpy: masks [H, G] uint64 on the packed grid, frame_off [R + 1], K [H, R] -> a dict of what the device
    path leaves: speakers [G, 2] int32, tallies [R, 4] int64, dis [R, H, H] int64, order [R, H], weight [R, H] int32, label_of
    [spk_off[-1]] int32 (group (h, r) at spk_off[h R + r]), n_labels [R], overflow [R] int32, and the pair tables co [co_off[-1]] int32,
    tally [P R, 2], correct [P R] int64 and mapping [row_off[-1]] int32 (one optimal map per pair group)."""
    tab = FuseTables(K, frame_off, "fuse_host")
    H, R, P = tab.H, tab.R, tab.P
    w = check_weights("fuse_host", None if weights is None else [int(x) for x in weights], H)
    cap = check_cap("fuse_host", cap)
    masks = np.asarray(masks, dtype=np.uint64).reshape(H, tab.G)
    out = {"speakers": np.full((tab.G, 2), -1, np.int32), "tallies": np.zeros((R, 4), np.int64), "dis": np.zeros((R, H, H), np.int64),
           "order": np.zeros((R, H), np.int32), "weight": np.zeros((R, H), np.int32), "label_of": np.full(tab.n_spk, -1, np.int32),
           "n_labels": np.zeros(R, np.int32), "overflow": np.zeros(R, np.int32), "co": np.zeros(tab.co_total, np.int32),
           "tally": np.zeros((P * R, 2), np.int64), "correct": np.zeros(P * R, np.int64), "mapping": np.full(tab.n_rows, -1, np.int32)}
    for r in range(R):
        a0, a1 = int(tab.frame_off[r]), int(tab.frame_off[r + 1])
        Kr = [int(k) for k in tab.K[:, r]]
        m = [masks[h, a0:a1] for h in range(H)]
        co = {}
        for p, (a, b) in enumerate(pairs(H)):
            q = p * R + r
            co[(a, b)], out["tally"][q] = cooccur_host(m[a], Kr[a], m[b], Kr[b])
            mapping, out["correct"][q] = assignment_host(co[(a, b)])
            out["co"][int(tab.co_off[q]):int(tab.co_off[q + 1])] = co[(a, b)].reshape(-1)
            out["mapping"][int(tab.row_off[q]):int(tab.row_off[q + 1])] = mapping
            out["dis"][r, a, b] = out["dis"][r, b, a] = out["tally"][q, 0] - out["correct"][q]
        out["order"][r], out["weight"][r], label_of, out["n_labels"][r], out["overflow"][r] = labels_host(co, out["dis"][r], Kr, w)
        for h in range(H):
            out["label_of"][int(tab.spk_off[h * R + r]):int(tab.spk_off[h * R + r + 1])] = label_of[h]
        out["speakers"][a0:a1], tal = vote_host(m, Kr, label_of, out["weight"][r], cap)
        out["tallies"][r] = [*tal, int(out["overflow"][r])]
    return out


# ------------------------------------------------------------------------------------------------ the device path
def _offsets(who: str, tab: FuseTables):
    from . import _args
    if tab.frame_off_d is None:
        raise ValueError(f"{who}: the tables are not on the device (FuseTables.to)")
    _args.tensor(who, "frame_off", tab.frame_off_d, "int32", (tab.R + 1,))
    _args.tensor(who, "spk_off", tab.spk_off_d, "int32", (tab.H * tab.R + 1,))
    _args.tensor(who, "co_off", tab.co_off_d, "int64", (tab.P * tab.R + 1,))


def fuse_masks(eng, speakers, tab: FuseTables, h: int, out=None):
    """speakers [G, 2] int32 on the packed grid (device): hypothesis h of every recording of tab -> mask [G] int64 holding the uint64 masks
    (out: where it is written): sdk_fuse_masks.  Nothing waits."""
    import torch
    from . import _args
    from ._lib import check
    from .ops import _stream
    who = "fuse_masks"
    if not 0 <= int(h) < tab.H:
        raise ValueError(f"{who}: h={h} (0 .. {tab.H - 1})")
    _offsets(who, tab)
    _args.tensor(who, "speakers", speakers, "int32", (tab.G, 2))
    if out is None:
        out = torch.empty((tab.G,), dtype=torch.int64, device=speakers.device)
    _args.tensor(who, "out", out, "int64", (tab.G,))
    spk_off = tab.spk_off_d[int(h) * tab.R:int(h) * tab.R + tab.R + 1]
    check(eng.lib.sdk_fuse_masks(eng.ctx, speakers.data_ptr() if tab.G else None, tab.frame_off_d.data_ptr(), spk_off.data_ptr(), tab.R, tab.G,
                                 int(tab.K[int(h)].max()), out.data_ptr() if tab.G else None, _stream()), "sdk_fuse_masks")
    return out


def fuse_cooccur(eng, mask, tab: FuseTables):
    """mask [H, G] int64 (device) -> (co [co_total] int32, tally [P R, 2] int64) on the device: sdk_fuse_cooccur.  Nothing waits."""
    import torch
    from . import _args
    from ._lib import check
    from .ops import _stream
    who = "fuse_cooccur"
    _offsets(who, tab)
    _args.tensor(who, "mask", mask, "int64", (tab.H, tab.G))
    co = torch.empty((max(tab.co_total, 1),), dtype=torch.int32, device=mask.device)
    tally = torch.empty((tab.P * tab.R, 2), dtype=torch.int64, device=mask.device)
    check(eng.lib.sdk_fuse_cooccur(eng.ctx, mask.data_ptr() if tab.G else None, tab.frame_off_d.data_ptr(), tab.spk_off_d.data_ptr(), tab.co_off_d.data_ptr(),
                                   tab.H, tab.R, tab.G, tab.max_spk, tab.co_total, co.data_ptr(), tally.data_ptr(), _stream()), "sdk_fuse_cooccur")
    return co[:tab.co_total], tally


def pair_map(eng, co, tab: FuseTables):
    """co of fuse_cooccur -> (mapping [row_off[-1]] int32, correct [P R] int64): sdk_score_map on the pair tables as they stand."""
    import torch
    from . import _args
    from ._lib import check
    from .ops import _stream
    who = "fuse.pair_map"
    _offsets(who, tab)
    _args.tensor(who, "co", co, "int32", (tab.co_total,))
    _args.tensor(who, "row_off", tab.row_off_d, "int32", (tab.P * tab.R + 1,))
    _args.tensor(who, "col_off", tab.col_off_d, "int32", (tab.P * tab.R + 1,))
    mapping = torch.empty((max(tab.n_rows, 1),), dtype=torch.int32, device=co.device)
    correct = torch.empty((tab.P * tab.R,), dtype=torch.int64, device=co.device)
    check(eng.lib.sdk_score_map(eng.ctx, co.data_ptr(), tab.row_off_d.data_ptr(), tab.col_off_d.data_ptr(), tab.co_off_d.data_ptr(), tab.P * tab.R, tab.max_spk,
                                tab.max_spk, mapping.data_ptr(), correct.data_ptr(), _stream()), "sdk_score_map")
    return mapping[:tab.n_rows], correct


def fuse_labels(eng, co, tally, correct, tab: FuseTables, weights=None):
    """co, tally of fuse_cooccur and correct of pair_map (device); weights: None (the rank table) or an [H] int32 device tensor -> (dis
    [R, H, H] int64, order [R, H], weight [R, H], label_of [spk_off[-1]], n_labels [R], overflow [R] int32) on the device:
    sdk_fuse_labels.  Nothing waits."""
    import torch
    from . import _args
    from ._lib import check
    from .ops import _stream
    who = "fuse_labels"
    H, R = tab.H, tab.R
    _offsets(who, tab)
    _args.tensor(who, "co", co, "int32", (tab.co_total,))
    _args.tensor(who, "tally", tally, "int64", (tab.P * R, 2))
    _args.tensor(who, "correct", correct, "int64", (tab.P * R,))
    _args.tensor(who, "rank_weight", tab.rank_weight_d, "int32", (MAX_FUSE_HYPS,))
    if weights is not None:
        _args.tensor(who, "weights", weights, "int32", (H,))
    dev = tally.device
    dis = torch.empty((R, H, H), dtype=torch.int64, device=dev)
    order, weight = (torch.empty((R, H), dtype=torch.int32, device=dev) for _ in range(2))
    label_of = torch.empty((max(tab.n_spk, 1),), dtype=torch.int32, device=dev)
    n_labels, overflow = (torch.empty((R,), dtype=torch.int32, device=dev) for _ in range(2))
    check(eng.lib.sdk_fuse_labels(eng.ctx, co.data_ptr(), tally.data_ptr(), correct.data_ptr(), tab.spk_off_d.data_ptr(), tab.co_off_d.data_ptr(),
                                  tab.rank_weight_d.data_ptr(), None if weights is None else weights.data_ptr(), H, R, tab.max_spk, dis.data_ptr(),
                                  order.data_ptr(), weight.data_ptr(), label_of.data_ptr(), n_labels.data_ptr(), overflow.data_ptr(), _stream()), "sdk_fuse_labels")
    return dis, order, weight, label_of[:tab.n_spk], n_labels, overflow


def fuse_vote(eng, mask, label_of, weight, overflow, tab: FuseTables, cap: int = 2):
    """mask [H, G] int64, and label_of, weight, overflow of fuse_labels (device) -> (speakers [G, 2] int32, tallies [R, 4] int64 = (speech,
    overlap, unanimous, overflow)) on the device: sdk_fuse_vote.  Nothing waits."""
    import torch
    from . import _args
    from ._lib import check
    from .ops import _stream
    who = "fuse_vote"
    cap = check_cap(who, cap)
    _offsets(who, tab)
    _args.tensor(who, "mask", mask, "int64", (tab.H, tab.G))
    _args.tensor(who, "label_of", label_of, "int32", (tab.n_spk,))
    _args.tensor(who, "weight", weight, "int32", (tab.R, tab.H))
    _args.tensor(who, "overflow", overflow, "int32", (tab.R,))
    speakers = torch.empty((tab.G, 2), dtype=torch.int32, device=mask.device)
    tallies = torch.empty((tab.R, 4), dtype=torch.int64, device=mask.device)
    check(eng.lib.sdk_fuse_vote(eng.ctx, mask.data_ptr() if tab.G else None, tab.frame_off_d.data_ptr(), tab.spk_off_d.data_ptr(),
                                label_of.data_ptr() if tab.n_spk else None, weight.data_ptr(), overflow.data_ptr(), tab.H, tab.R, tab.G, tab.max_spk, cap,
                                speakers.data_ptr() if tab.G else None, tallies.data_ptr(), _stream()), "sdk_fuse_vote")
    return speakers, tallies


def fuse_tables(eng, mask, tab: FuseTables, weights=None, cap: int = 2) -> dict:
    """mask [H, G] int64 on the device -> every table of fuse_host, by the same names, on the device: the calls behind sdk_fuse_masks in
    stream order.  Nothing is read back."""
    co, tally = fuse_cooccur(eng, mask, tab)
    mapping, correct = pair_map(eng, co, tab)
    dis, order, weight, label_of, n_labels, overflow = fuse_labels(eng, co, tally, correct, tab, weights)
    speakers, tallies = fuse_vote(eng, mask, label_of, weight, overflow, tab, cap)
    return {"speakers": speakers, "tallies": tallies, "dis": dis, "order": order, "weight": weight, "label_of": label_of, "n_labels": n_labels,
            "overflow": overflow, "co": co, "tally": tally, "correct": correct, "mapping": mapping}


def download(tables: dict) -> dict:
    """The device tables of fuse_tables -> numpy, in one download."""
    import torch
    flat = torch.cat([t.reshape(-1).to(torch.int64) for t in tables.values()]).cpu().numpy()
    out, a = {}, 0
    for name, t in tables.items():
        out[name] = flat[a:a + t.numel()].reshape(tuple(t.shape)).astype(str(t.dtype).rpartition(".")[2])
        a += t.numel()
    return out


# ------------------------------------------------------------------------------------------------ hypotheses in, results out
@dataclass
class FusedDiarization:
    """What fuse_results returns for a recording whose anchor is a turn list (an anchor that is a DiarizationResult is copied instead)."""
    turns: list                               # (start_s, end_s, label), by start then label
    n_speakers: int                           # the fused labels
    speakers: np.ndarray                      # [G, 2] int32, padded with -1
    fusion: Optional[dict] = None


def is_hypothesis(x) -> bool:
    """A result (speakers and n_speakers) or a turn list [(start_s, end_s, name)]."""
    if hasattr(x, "speakers") and hasattr(x, "n_speakers"):
        return True
    return isinstance(x, (list, tuple)) and all(isinstance(t, (list, tuple)) and len(t) == 3 and isinstance(t[0], numbers.Real) for t in x)


class _Pack:
    """The hypotheses of a call, checked on the host: prepare()."""


def prepare(who: str, hypotheses, n_samples=None) -> _Pack:
    """hypotheses[r][h] -> the pack's host tables; every refusal of the module docstring's "inputs" is a ValueError raised here."""
    hyps = [list(rec) for rec in hypotheses]
    R = len(hyps)
    if R and len({len(rec) for rec in hyps}) != 1:
        raise ValueError(f"{who}: every recording needs the same number of hypotheses, got {[len(rec) for rec in hyps][:8]}")
    H = _check_hyps(who, len(hyps[0]) if R else 2)
    if n_samples is not None and isinstance(n_samples, numbers.Integral):
        n_samples = [n_samples]
    if n_samples is not None and len(n_samples) != R:
        raise ValueError(f"{who}: {len(n_samples)} entries of n_samples for {R} recordings")
    pk = _Pack()
    pk.H, pk.R, pk.G_r, pk.kind, pk.sp, pk.turns, pk.names = H, R, [], [], [], [], []
    K = np.zeros((H, max(R, 1)), np.int64)
    for r, rec in enumerate(hyps):
        G = None if n_samples is None or n_samples[r] is None else global_frames(int(n_samples[r]))
        kind, sps, turns, names = [], [], [], []
        for h, x in enumerate(rec):
            if not is_hypothesis(x):
                raise ValueError(f"{who}: recording {r}, hypothesis {h}: a result (speakers, n_speakers) or a list of (start_s, end_s, name), got {type(x).__name__}")
            if hasattr(x, "speakers"):
                sp = np.ascontiguousarray(x.speakers, dtype=np.int32).reshape(-1, 2)
                if G is not None and len(sp) != G:
                    raise ValueError(f"{who}: recording {r}: hypothesis {h} holds {len(sp)} frames, the others (or n_samples) give {G}")
                G = len(sp)
                K[h, r] = max(int(x.n_speakers), 0)
                kind.append("result"), sps.append(sp), turns.append(None), names.append(None)
            else:
                merged, nm = prepare_reference(x)
                K[h, r] = len(nm)
                kind.append("turns"), sps.append(None), turns.append(merged), names.append(nm)
            if K[h, r] > MAX_FUSE_SPEAKERS:
                raise ValueError(f"{who}: recording {r}, hypothesis {h}: {int(K[h, r])} speakers; at most {MAX_FUSE_SPEAKERS}")
        if G is None:
            raise ValueError(f"{who}: recording {r} has turn lists only: pass n_samples, the recording's length")
        pk.G_r.append(G), pk.kind.append(kind), pk.sp.append(sps), pk.turns.append(turns), pk.names.append(names)
    pk.tab = FuseTables(K, np.concatenate([[0], np.cumsum(pk.G_r)]), who) if R else None
    return pk


def masks_of(pk: _Pack) -> np.ndarray:
    """The pack's masks [H, G] uint64 on the host (what the device path rasterises)."""
    tab = pk.tab
    out = np.zeros((tab.H, tab.G), np.uint64)
    for r in range(tab.R):
        a, b = int(tab.frame_off[r]), int(tab.frame_off[r + 1])
        for h in range(tab.H):
            if pk.kind[r][h] == "result":
                out[h, a:b] = masks_host(pk.sp[r][h], int(tab.K[h, r]))
            else:
                from .score import reference_masks_host
                out[h, a:b] = reference_masks_host(pk.turns[r][h], b - a)[0]
    return out


def _run(eng, pk: _Pack, weights, cap: int) -> dict:
    """One upload, the calls, one download -> fuse_host's tables in numpy."""
    import torch
    from ._lib import check
    from .ops import _stream
    tab = pk.tab
    H, R, G = tab.H, tab.R, tab.G
    parts = tab.host_parts()
    if weights is not None:
        parts.append(weights)
    if sum(len(p) for p in parts) & 1:
        parts.append(np.zeros(1, np.int32))                                                          # the speakers tables are read as int2: 8-byte aligned
    sp_at = sum(len(p) for p in parts)
    sp_all = np.full((H, G, 2), -1, np.int32)
    for r in range(R):
        for h in range(H):
            if pk.kind[r][h] == "result":
                sp_all[h, int(tab.frame_off[r]):int(tab.frame_off[r + 1])] = pk.sp[r][h]
    parts.append(sp_all.reshape(-1))
    turn_h = [h for h in range(H) if any(pk.kind[r][h] == "turns" for r in range(R))]
    M_h = {}
    for h in turn_h:
        rows = [pk.turns[r][h] if pk.kind[r][h] == "turns" else np.zeros((0, 3), np.int32) for r in range(R)]
        M_h[h] = sum(len(t) for t in rows)
        if M_h[h] >= 1 << 28:
            raise ValueError(f"fuse: {M_h[h]} turns in one pack (fewer than 2^28)")
        parts += [np.concatenate([[0], np.cumsum([len(t) for t in rows])]).astype(np.int32)] + [t.reshape(-1).astype(np.int32) for t in rows]
    up = torch.from_numpy(np.concatenate(parts)).to(eng.device)                                                                          # one upload
    at = tab.bind(up)
    w_d = None if weights is None else up[at:at + H]
    sp_d = up[sp_at:sp_at + 2 * H * G].reshape(H, G, 2)
    at = sp_at + 2 * H * G
    mask = torch.empty((H, G), dtype=torch.int64, device=eng.device)
    tmp = scored = None
    for h in range(H):
        if any(pk.kind[r][h] == "result" for r in range(R)):
            fuse_masks(eng, sp_d[h], tab, h, out=mask[h])
        if h in turn_h:
            turn_off_d, turns_d = up[at:at + R + 1], up[at + R + 1:at + R + 1 + 3 * M_h[h]]
            at += R + 1 + 3 * M_h[h]
            everyone = all(pk.kind[r][h] == "turns" for r in range(R))
            if scored is None:
                scored = torch.empty((max(G, 1),), dtype=torch.uint8, device=eng.device)
                tmp = torch.empty((max(G, 1),), dtype=torch.int64, device=eng.device)
            dst = mask[h] if everyone else tmp
            check(eng.lib.sdk_score_reference(eng.ctx, turns_d.data_ptr() if M_h[h] else None, turn_off_d.data_ptr(), tab.frame_off_d.data_ptr(),
                                              tab.spk_off_d[h * R:h * R + R + 1].data_ptr(), R, M_h[h], G, int(tab.K[h].max()), 0, 0,
                                              dst.data_ptr() if G else None, scored.data_ptr() if G else None, _stream()), "sdk_score_reference")
            if not everyone:
                for r in range(R):
                    if pk.kind[r][h] == "turns":
                        a, b = int(tab.frame_off[r]), int(tab.frame_off[r + 1])
                        mask[h, a:b].copy_(tmp[a:b])
    return download(fuse_tables(eng, mask, tab, w_d, cap))                                                                              # one download


def _label_dict(pk: _Pack, out: dict, r: int, h: int) -> dict:
    tab = pk.tab
    lab = out["label_of"][int(tab.spk_off[h * tab.R + r]):int(tab.spk_off[h * tab.R + r + 1])]
    keys = pk.names[r][h] if pk.kind[r][h] == "turns" else range(len(lab))
    return {k: int(u) for k, u in zip(keys, lab)}


def _cap_of(who: str, max_speakers) -> int:
    if max_speakers is not None and int(max_speakers) < 0:
        raise ValueError(f"{who}: max_speakers={max_speakers}: must be None or >= 0")
    return max(_speaker_cap(max_speakers), 1)


def assemble(pk: _Pack, hypotheses, out: dict) -> list:
    """fuse_host's tables (host or downloaded) -> one result per recording ("fuse_results")."""
    tab, res = pk.tab, []
    for r in range(tab.R):
        a, b = int(tab.frame_off[r]), int(tab.frame_off[r + 1])
        anchor, L = int(out["order"][r][0]), int(out["n_labels"][r])
        speakers = np.ascontiguousarray(out["speakers"][a:b], dtype=np.int32)
        fusion = {"order": [int(h) for h in out["order"][r]], "weights": [int(w) for w in out["weight"][r]], "dis": np.asarray(out["dis"][r], dtype=np.int64).copy(),
                  "label_of": [_label_dict(pk, out, r, h) for h in range(tab.H)], "speech": int(out["tallies"][r][0]), "overlap": int(out["tallies"][r][1]),
                  "unanimous": int(out["tallies"][r][2]), "overflow": int(out["tallies"][r][3])}
        src = list(hypotheses[r])[anchor]
        if pk.kind[r][anchor] == "result":
            new = copy.copy(src)
            new.speakers, new.turns, new.n_speakers, new.fusion = speakers, turns_from_frames(speakers, L), L, fusion
        else:
            new = FusedDiarization(turns_from_frames(speakers, L), L, speakers, fusion)
        res.append(new)
    return res


def fuse_results(eng, hypotheses, n_samples=None, weights=None, max_speakers=None) -> list:
    """Backend.fuse_diarizations: hypotheses[r][h], the H hypotheses of every recording (each a DiarizationResult, or a turn list
    [(start_s, end_s, name)]), n_samples: the recordings' lengths (needed where a recording has turn lists only) -> one fused result per
    recording: a copy of the anchor's result where the anchor is one (its centroids keep the anchor's numbers, which the fused labels below
    K_anchor share), else a FusedDiarization; speakers, turns (turns_from_frames) and n_speakers = the fused labels are replaced and
    `fusion` = {order, weights, dis, label_of (per hypothesis: own speaker or name -> fused label, -1: overflow), speech, overlap,
    unanimous, overflow} is added.  weights: None (rank weights) or H integers in 1 .. 65536; max_speakers caps the speakers per frame as
    in diarize.  One upload, the device calls, one download."""
    hypotheses = [list(rec) for rec in hypotheses]
    pk = prepare("fuse", hypotheses, n_samples)
    w = check_weights("fuse", weights, pk.H)
    cap = _cap_of("fuse", max_speakers)
    if not pk.R:
        return []
    return assemble(pk, hypotheses, _run(eng, pk, w, cap))


def compare(eng, a, b, n_samples=None) -> List[dict]:
    """Backend.compare_diarizations: the pairwise part alone, for two hypotheses per recording (a[r], b[r]) -> one dict per recording: co
    [K_a, K_b] int32, mapping [K_a] int32 (b's speaker for each of a's in an assignment that attains `correct`, -1: none), names_a,
    names_b (a turn list's names in speaker order, None for a result), sum_max, sum_min, correct, disagreement = (sum_max - correct) /
    sum_max (0.0 when sum_max is 0) and unanimous, the frames in which both name the same fused labels."""
    a, b = list(a), list(b)
    if len(a) != len(b):
        raise ValueError(f"compare: {len(a)} and {len(b)} hypotheses")
    pk = prepare("compare", [[x, y] for x, y in zip(a, b)], n_samples)
    if not pk.R:
        return []
    out, tab, res = _run(eng, pk, None, 2), pk.tab, []
    for r in range(tab.R):
        Ka, Kb = int(tab.K[0, r]), int(tab.K[1, r])
        smax, smin, correct = int(out["tally"][r][0]), int(out["tally"][r][1]), int(out["correct"][r])
        res.append({"co": out["co"][int(tab.co_off[r]):int(tab.co_off[r + 1])].reshape(Ka, Kb).astype(np.int32),
                    "mapping": out["mapping"][int(tab.row_off[r]):int(tab.row_off[r + 1])].astype(np.int32), "names_a": pk.names[r][0], "names_b": pk.names[r][1],
                    "sum_max": smax, "sum_min": smin, "correct": correct, "disagreement": (smax - correct) / smax if smax else 0.0,
                    "unanimous": int(out["tallies"][r][2])})
    return res


# ---- fusing several diarizations of a recording.  Functions of a Backend (backend.py), not methods of it: the class keeps its public names;
#      backend.py imports them, so callers reach them as backend.fuse_diarizations and so on.
def _per_recording(x) -> bool:
    """True where x is a list over recordings, False where it is one hypothesis (a result, or a non-empty turn list)."""
    from .fuse import is_hypothesis
    return not (is_hypothesis(x) and not (isinstance(x, (list, tuple)) and len(x) == 0))


def fuse_diarizations(be: Backend, hypotheses, n_samples=None, weights=None, max_speakers=None):
    """Several diarizations of the same recordings combined into one each, DOVER-Lap's way: hypotheses[r] = the H (2 .. 8) answers for
    recording r, each a diarize.DiarizationResult (of diarize / diarize_many under different models, clusterings or thresholds) or a turn
    list [(start_s, end_s, name)] (an outside diarizer's; then n_samples, the recordings' lengths, fixes the frame grid where no result
    does).  The speakers of the hypotheses are mapped onto common labels through their pairwise co-occurrence, starting from the hypothesis
    that agrees most with the others; the hypotheses are weighted by their rank in mean disagreement (or by weights=, H integers in
    1 .. 65536) and every frame is voted, the number of speakers from the weighted mean count (at most 2, fewer with max_speakers).  -> one
    result per recording: the anchor's result copied (else a fuse.FusedDiarization) with speakers, turns and n_speakers replaced and
    `fusion` = {order, weights, dis, label_of, speech, overlap, unanimous, overflow}.  One upload, the device calls and one download for
    the whole list (fuse.py states the rule; parity with DOVER-Lap is unpinned)."""
    from .fuse import fuse_results
    return fuse_results(be.engine(), list(hypotheses), n_samples, weights, max_speakers)


def compare_diarizations(be: Backend, a, b, n_samples=None):
    """Two diarizations of the same recording laid side by side: a and b are one hypothesis each (as fuse_diarizations takes them), or
    lists of them, one per recording -> per recording a dict of co [K_a, K_b] (the frames speaker i of a shares with speaker j of b), mapping
    (b's speaker for each of a's under an optimal assignment), names_a, names_b, sum_max, sum_min, correct, disagreement = (sum_max -
    correct) / sum_max - the symmetric diarization error of one against the other, 0.0 for two silent answers - and unanimous, the frames
    on which they agree.  A single pair gives a single dict."""
    from .fuse import compare
    single = not _per_recording(a)
    if single:
        a, b = [a], [b]
        n_samples = None if n_samples is None else [n_samples]
    out = compare(be.engine(), a, b, n_samples)
    return out[0] if single else out


def diarize_fused(be: Backend, samples_or_path, variants, **fuse_kw):
    """diarize once per keyword set of `variants` (for example [{"clustering": "ahc"}, {"clustering": "vbx", "threshold": 0.6},
    {"clustering": "nmesc"}]) and the results fused (fuse_diarizations; fuse_kw: weights, max_speakers) -> the fused result.  Every
    variant runs the whole pipeline: the embedding pass is not shared between them."""
    variants = [dict(v) for v in variants]
    from .fuse import MAX_FUSE_HYPS
    if not 2 <= len(variants) <= MAX_FUSE_HYPS:
        raise ValueError(f"diarize_fused: {len(variants)} variants (2 .. {MAX_FUSE_HYPS})")
    samples, = be._recordings([samples_or_path])                 # a path is decoded once, not per variant
    return fuse_diarizations(be, [[be.diarize(samples, **v) for v in variants]], **fuse_kw)[0]
