"""The host layer of the diarization: its constants, DiarizationResult, the packing of many recordings (Pack, pack_recordings) and the rule of
diarize.py's module docstring restated in numpy - the *_host functions say what the kernels of csrc/diarize.hip compute, for hosts that
post-process stored class tables and for the tests.  numpy and segmentation.py only: no torch, no library, no other module of the pipeline,
so diarize_ops.py, cluster.py, score.py and stream.py can all import it.  diarize.py re-exports every name."""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from .segmentation import CHUNK, FRAME_FIRST, FRAME_HOP, POWERSET, chunk_starts, frames_to_ranges
from .segmentation import num_frames as seg_frames

MIN_CLEAN_COLUMNS = 4            # ours (~0.32 s of the last map): below it the overlapped columns are kept
MIN_VALID_COLUMNS = 2            # the unbiased variance needs two columns
TRAIN_CLEAN_DEN = 5              # ours, after PyAnnote's filter: a training row has clean_frames >= F / 5
MAX_LINKAGE_ROWS = 65536         # Engine.centroid_linkage serves N <= 65 536
DEFAULT_BATCH = 128              # $SDK_DIARIZE_BATCH: chunks per forward (the ResNet workspace is ~15 MB per chunk at T = 1001)
N_LOCAL = 3                      # local speakers of the powerset
MAX_ASSIGN_DIM = 512             # sdk_diarize_centroids / sdk_diarize_assign serve d = 64, 128, .. 512

_MASK = np.array([[k in cls for k in range(N_LOCAL)] for cls in POWERSET], dtype=bool)       # [7, 3]
_COUNT = _MASK.sum(1).astype(np.int64)


@dataclass
class DiarizationResult:
    turns: List[Tuple[float, float, int]]     # (start_s, end_s, speaker), by start then speaker
    n_speakers: int
    centroids: np.ndarray                     # [K, embed_dim] unit fp32, in the space of the Diarizer's embedder: that of score_windows and enrolled profiles under SDK_MODEL=resnet34, or SDK_MODEL=ecapa with SDK_DIARIZE_MODEL=ecapa (backend.py)
    labels: np.ndarray                        # [C, 3] int32: cluster of every (chunk, local speaker), -1: none
    count: np.ndarray                         # [G] uint8 speakers per global frame
    speakers: np.ndarray                      # [G, 2] int32, padded with -1
    starts: np.ndarray                        # [C] int64 first samples of the chunks
    info: np.ndarray                          # [C, 3, 4] int32 (active frames, clean frames, used_clean, valid)
    cls: object = None                        # [C, F] uint8 class table (device tensor; None for an empty recording)
    scores: Optional[np.ndarray] = None       # [C, 3] fp32 cosine of every assigned row to its centroid, 0 where the label is -1 (constrained=True, or clustering="vbx")
    # clustering="vbx" sets these two on the result (None otherwise).  Plain attributes with a class default, not dataclass fields: the
    # field list, and with it the positional constructor, ends with scores as before.
    pi = None                                 # [S] float64 weights of the S initial speakers after the last iteration
    elbo = None                               # [n_iter] float64
    nmesc = None                              # clustering="nmesc": {p, k, ps, eigenvalues [n_p, m], ratios [n_p]} of cluster.nmesc_cluster ("nmesc" in diarize.py); else None
    smoothing = None                          # min_duration_off / min_duration_on above 0: {min_duration_off, min_duration_on, fill, keep, filled, dropped} ("smoothing" in diarize.py, smooth.py); else None
    forced = None                             # speakers= overruled the clustering: {found, target, method, level, n_iter} ("bounds" in diarize.py); else None


# ------------------------------------------------------------------------------------------------ host restatements (numpy, vectorised)
def global_frames(n_samples: int) -> int:
    return max(0, (int(n_samples) - FRAME_FIRST + FRAME_HOP - 1) // FRAME_HOP)


def decode_host(logp: np.ndarray) -> np.ndarray:
    """logp [..., 7] -> uint8 argmax class (numpy's first maximum: ties to the lower class).  NaN as in sdk_powerset_decode, whose scan keeps
    the best so far unless a class is greater: a NaN in class 0 keeps class 0, a NaN elsewhere is never taken."""
    logp = np.asarray(logp)
    nan = np.isnan(logp)
    if nan.any():
        logp = np.where(nan, -np.inf, logp)
        logp[..., 0] = np.where(nan[..., 0], np.inf, logp[..., 0])
    return np.argmax(logp, axis=-1).astype(np.uint8)


def masks_host(cls: np.ndarray, T4: int):
    """cls [B, F] -> (w [B, 3, T4] fp32, info [B, 3, 4] int32): sdk_diarize_masks."""
    cls = np.asarray(cls)
    B, F = cls.shape
    active = _MASK[cls]                                                  # [B, F, 3]
    alone = (_COUNT[cls] < 2)[:, :, None]
    col = np.minimum(F - 1, (np.arange(T4, dtype=np.int64) * F) // T4)
    full = active[:, col, :].transpose(0, 2, 1)                           # [B, 3, T4]
    clean = (active & alone)[:, col, :].transpose(0, 2, 1)
    used = clean.sum(2) >= MIN_CLEAN_COLUMNS
    w = np.where(used[:, :, None], clean, full)
    info = np.stack([active.sum(1), (active & alone).sum(1), used, w.sum(2) >= MIN_VALID_COLUMNS], axis=2).astype(np.int32)
    return w.astype(np.float32), info


def reconstruct_host(cls: np.ndarray, starts: np.ndarray, labels: np.ndarray, K: int, n_samples: int, max_speakers: Optional[int] = None):
    """sdk_diarize_reconstruct in numpy -> (count [G] uint8, speakers [G, 2] int32, act [G, K] int32, nc [G] int64)."""
    cls, labels = np.asarray(cls), np.asarray(labels)
    Cn, F = cls.shape
    G = global_frames(n_samples)
    cap = _speaker_cap(max_speakers)
    act = np.zeros((G, K), np.int32)
    cnt, nc = np.zeros(G, np.int64), np.zeros(G, np.int64)
    for c in range(Cn):
        q = (135 - int(starts[c])) // FRAME_HOP
        g = np.arange(F) - q
        m = (g >= 0) & (g < G)
        cnt[g[m]] += _COUNT[cls[c][m]]
        nc[g[m]] += 1
        on = _MASK[cls[c][m]]                                             # [frames, 3]
        for k in {int(v) for v in labels[c] if 0 <= v < K}:              # a label at or above K names no cluster: it counts, but for no act
            act[g[m], k] += on[:, labels[c] == k].any(1)
    count = np.where(nc > 0, np.minimum((2 * cnt + nc) // np.maximum(2 * nc, 1), cap), 0)
    order = np.argsort(-act, axis=1, kind="stable")[:, :2] if K else np.zeros((G, 0), np.int64)      # stable: ties to the lower cluster
    speakers = np.full((G, 2), -1, np.int32)
    for slot in range(min(2, K)):
        k = order[:, slot]
        ok = (count > slot) & (act[np.arange(G), k] > 0)
        speakers[ok, slot] = k[ok]
    return count.astype(np.uint8), speakers, act, nc


def _speaker_cap(max_speakers: Optional[int]) -> int:     # speakers per frame: the powerset's 2, fewer when max_speakers says so
    return 2 if max_speakers is None else min(2, int(max_speakers))


def candidate_mask(info: np.ndarray) -> np.ndarray:
    """bool per row (c * 3 + s): a candidate of the assignment, valid and with an active frame."""
    i = np.asarray(info).reshape(-1, 4)
    return (i[:, 3] != 0) & (i[:, 0] > 0)


def training_mask(info: np.ndarray, F: int) -> np.ndarray:
    """bool per row (c * 3 + s): in the clustering's training set, valid and TRAIN_CLEAN_DEN * clean_frames >= F."""
    i = np.asarray(info).reshape(-1, 4)
    return (i[:, 3] != 0) & (TRAIN_CLEAN_DEN * i[:, 1].astype(np.int64) >= F)


def training_rows(info: np.ndarray, F: int) -> np.ndarray:
    """Rows (c * 3 + s) of the clustering's training set (training_mask)."""
    return np.flatnonzero(training_mask(info, F))


def reference_labels(cls: np.ndarray, info: np.ndarray, starts: np.ndarray, ref_mask: np.ndarray, n_ref: int) -> np.ndarray:
    """The reference speaker of every row (c * 3 + s) of one recording, for training a PLDA (Diarizer.plda_rows), in integers on the host.
    cls [C, F] uint8, info [C, 3, 4], starts [C] the chunks' first samples, ref_mask [G] uint64 (score.reference_masks_host, no collar: bit r
    = reference speaker r is active in global frame g), n_ref speakers.  A row outside training_mask gets -1.  A training row: over the chunk
    frames i where its local speaker is active and the frame's count is < 2, mapped to g = i - q_c (the stitching's map,
    q_c = (135 - start_c) // 270) and kept where 0 <= g < G, tally per reference speaker the frames in which that speaker is active; the row
    takes the speaker of the largest tally (ties to the lower index) if 2 * tally >= the number of those frames, else -1."""
    cls, starts = np.asarray(cls), np.asarray(starts, dtype=np.int64)
    Cn, F = cls.shape
    G = int(len(ref_mask))
    train = training_mask(info, F)
    out = np.full(Cn * N_LOCAL, -1, np.int32)
    bit = np.uint64(1) << np.arange(max(int(n_ref), 1), dtype=np.uint64)
    for c in range(Cn):
        if not train[N_LOCAL * c:N_LOCAL * (c + 1)].any() or not n_ref:
            continue
        g = np.arange(F, dtype=np.int64) - (135 - int(starts[c])) // FRAME_HOP
        ok = (g >= 0) & (g < G) & (_COUNT[cls[c]] < 2)
        for s in range(N_LOCAL):
            if not train[N_LOCAL * c + s]:
                continue
            sel = ok & _MASK[cls[c]][:, s]
            n = int(sel.sum())
            if n == 0:
                continue
            tally = ((np.asarray(ref_mask, dtype=np.uint64)[g[sel]][:, None] & bit[None, :]) != 0).sum(0)
            best = int(np.argmax(tally))                                 # the first maximum: ties to the lower index
            if 2 * int(tally[best]) >= n:
                out[N_LOCAL * c + s] = best
    return out


def pack_rows(info: np.ndarray, chunk_off: np.ndarray):
    """Per recording of a pack: the rows that make its centroids (global rows of E, ascending) and how many of them are training rows."""
    cand_ok, train_ok = candidate_mask(info), training_mask(info, seg_frames(CHUNK))
    rows, n_train = [], []
    for r in range(len(chunk_off) - 1):
        a, b = N_LOCAL * int(chunk_off[r]), N_LOCAL * int(chunk_off[r + 1])
        tr = a + np.flatnonzero(train_ok[a:b])
        n_train.append(len(tr))
        rows.append(tr if len(tr) else a + np.flatnonzero(cand_ok[a:b]))      # no training row: one cluster of the candidates
    return rows, n_train


def _training_centroids(E64: np.ndarray, train: np.ndarray, train_labels: np.ndarray) -> np.ndarray:
    """The float64 mean of every cluster's training rows [K, d], added in ascending row order; not yet normalised."""
    K = int(np.max(train_labels)) + 1
    cent = np.zeros((K, E64.shape[1]))
    np.add.at(cent, np.asarray(train_labels, dtype=np.int64), E64[train])
    cent /= np.bincount(train_labels, minlength=K)[:, None]
    return cent


def assign_rows(E: np.ndarray, info: np.ndarray, train: np.ndarray, train_labels: np.ndarray):
    """Unit rows E [C * 3, d], info, the training rows and their cluster labels -> (labels [C, 3] int32, centroids [K, d] fp32 unit)."""
    E64 = np.asarray(E, dtype=np.float64)
    ok = candidate_mask(info)
    cand = np.flatnonzero(ok)
    labels = np.full(ok.size, -1, np.int32)
    if len(train):
        cent = _training_centroids(E64, train, train_labels)
    elif len(cand):
        cent = E64[cand].mean(0, keepdims=True)                           # numpy's pairwise mean; _centroids64 adds in row order instead
    else:
        return labels.reshape(-1, N_LOCAL), np.zeros((0, E64.shape[1]), np.float32)
    cent /= np.maximum(np.linalg.norm(cent, axis=1, keepdims=True), 1e-300)
    if len(cand):
        labels[cand] = np.argmax(E64[cand] @ cent.T, axis=1)              # first maximum: ties to the lowest centroid
    return labels.reshape(-1, N_LOCAL), cent.astype(np.float32)


def _centroids64(E64: np.ndarray, cand: np.ndarray, train: np.ndarray, train_labels: np.ndarray) -> np.ndarray:
    """The float64 unit centroids of assign_rows ([0, d] when there is neither a training row nor a candidate)."""
    if len(train):
        cent = _training_centroids(E64, train, train_labels)
    elif len(cand):
        cent = np.zeros((1, E64.shape[1]))
        np.add.at(cent, np.zeros(len(cand), np.int64), E64[cand])         # added in ascending row order, as the training rows are
        cent /= len(cand)
    else:
        return np.zeros((0, E64.shape[1]))
    return cent / np.maximum(np.linalg.norm(cent, axis=1, keepdims=True), 1e-300)


def constrained_chunk(cos: np.ndarray) -> Tuple[int, ...]:
    """cos [m, K] float64, the cosines of one chunk's m candidates (slot order) -> their m labels under the constrained rule."""
    import itertools
    m, K = cos.shape
    n = min(m, K)
    top = np.argsort(-cos, axis=1, kind="stable")[:, :min(3, K)]          # stable: ties to the lower cluster
    opts = [[int(k) for k in top[i] if cos[i, k] == cos[i, k]] + ([-1] if K < m else []) for i in range(m)]
    best, best_key, best_lab = None, None, (-1,) * m
    for lab in itertools.product(*opts):
        used = [k for k in lab if k >= 0]
        if len(used) != n or len(set(used)) != n:
            continue
        tot = 0.0
        for i, k in enumerate(lab):                                       # summed in slot order
            if k >= 0:
                tot = tot + cos[i, k]
        key = tuple(k if k >= 0 else K for k in lab)                      # -1 after every cluster
        if best is None or tot > best or (tot == best and key < best_key):
            best, best_key, best_lab = tot, key, lab
    return best_lab


def assign_constrained_host(E: np.ndarray, info: np.ndarray, train: np.ndarray, train_labels: np.ndarray):
    """assign_rows with the constrained rule (the module docstring; sdk_diarize_centroids + sdk_diarize_assign with constrained = 1 in numpy)
    -> (labels [C, 3] int32, centroids [K, d] fp32 unit).  Every cosine is one float64 sum over the columns of its own row, so equal rows
    have equal cosines."""
    ok = candidate_mask(info).reshape(-1, N_LOCAL)
    Cn = ok.shape[0]
    cand = np.flatnonzero(ok.reshape(-1))
    E32 = np.asarray(E)
    E64 = np.zeros(E32.shape, np.float64)
    E64[cand] = E32[cand]                                                # rows that are no candidates are never read
    train = np.asarray(train, dtype=np.int64)
    E64[train] = E32[train]
    cent = _centroids64(E64, cand, train, np.asarray(train_labels))
    labels = np.full((Cn, N_LOCAL), -1, np.int32)
    if cent.shape[0]:
        for c in np.flatnonzero(ok.any(1)):
            slots = np.flatnonzero(ok[c])
            cos = (E64[c * N_LOCAL + slots][:, None, :] * cent[None, :, :]).sum(-1)
            labels[c, slots] = constrained_chunk(cos)
    return labels, cent.astype(np.float32)


def appearance_order(speakers: np.ndarray, K: int) -> np.ndarray:
    """new id of every provisional cluster: by first appearance in speakers [G, 2] (frame order, then slot order); clusters that never
    appear follow in their old order."""
    flat = np.asarray(speakers).reshape(-1)
    flat = flat[flat >= 0]
    _, first = np.unique(flat, return_index=True)
    seen = flat[np.sort(first)]
    rest = np.setdiff1d(np.arange(K), seen)
    new = np.empty(K, np.int64)
    new[np.concatenate([seen, rest]).astype(np.int64)] = np.arange(K)
    return new


def turns_from_frames(speakers: np.ndarray, K: int) -> List[Tuple[float, float, int]]:
    out = []
    sp = np.asarray(speakers)
    for k in range(K):
        out += [(a, b, k) for a, b in frames_to_ranges((sp == k).any(1))]
    return sorted(out, key=lambda t: (t[0], t[2]))


def to_rttm(turns, uri: str) -> str:
    """Standard RTTM: one `SPEAKER <uri> 1 <start> <dur> <NA> <NA> SPEAKER_%02d <NA> <NA>` line per turn, 3 decimals."""
    return "".join(f"SPEAKER {uri} 1 {a:.3f} {b - a:.3f} <NA> <NA> SPEAKER_{k:02d} <NA> <NA>\n" for a, b, k in turns)


# ------------------------------------------------------------------------------------------------ many recordings: packing and the grouped rules
MAX_PACK_SAMPLES = (1 << 31) - 1 # starts are int32
DEFAULT_PACK_SAMPLES = 1 << 28   # $SDK_DIARIZE_PACK_SAMPLES: samples per pack of run_many (gaps included)
DEFAULT_PACK_LINKAGE_BYTES = 1 << 34   # $SDK_DIARIZE_PACK_LINKAGE_BYTES: bound on the grouped linkage's distance matrices, 8 (3 C_r)^2 bytes per recording


@dataclass
class Pack:
    """Recordings laid end to end (pack_recordings)."""
    samples: np.ndarray          # int16: recording r at rec_off[r], at least CHUNK zeros behind every recording
    starts_packed: np.ndarray    # [C] int32 chunk starts inside samples
    starts_local: np.ndarray     # [C] int32 chunk starts inside their own recording (chunk_starts; ascending per recording)
    chunk_off: np.ndarray        # [R + 1] int64 prefix sums of the chunks
    frame_off: np.ndarray        # [R + 1] int64 prefix sums of global_frames(n_r)
    n_samples: np.ndarray        # [R] int64
    rec_off: np.ndarray          # [R] int64 first sample of every recording inside samples


def pack_recordings(recordings, step_s: float = 1.0) -> Pack:
    """16 kHz mono int16 arrays -> Pack.  sdk_segmentation_forward and sdk_fbank_windows cut chunks from a start table and read zeros past the
    end of the buffer; with CHUNK zeros behind every recording a chunk that runs past its recording's end (a recording below 10 s) reads
    zeros exactly as it does alone and never the next recording.  An empty recording has no chunk and no frame."""
    xs = [np.ascontiguousarray(x, dtype=np.int16).reshape(-1) for x in recordings]
    n = np.array([x.size for x in xs], np.int64)
    rec_off = np.concatenate([[0], np.cumsum(n + CHUNK)]).astype(np.int64)
    if rec_off[-1] > MAX_PACK_SAMPLES:
        raise ValueError(f"pack_recordings: {int(rec_off[-1])} samples with the gaps; a pack holds fewer than 2^31 (the chunk starts are int32)")
    buf = np.zeros(int(rec_off[-1]), np.int16)
    local = [chunk_starts(int(m), step_s) if m else np.zeros(0, np.int64) for m in n]
    for x, o in zip(xs, rec_off):
        buf[o:o + x.size] = x
    packed = [st + o for st, o in zip(local, rec_off)]
    cat = (lambda v: np.concatenate(v) if v else np.zeros(0, np.int64))
    return Pack(buf, cat(packed).astype(np.int32), cat(local).astype(np.int32), np.concatenate([[0], np.cumsum([len(v) for v in local])]).astype(np.int64),
                np.concatenate([[0], np.cumsum([global_frames(int(m)) for m in n])]).astype(np.int64), n, rec_off[:-1].copy())


def split_packs(sizes, n_chunks) -> List[List[int]]:
    """The recordings' sample and chunk counts -> [[recording index]] per pack, in order: a pack is closed before the recording that would
    take it past $SDK_DIARIZE_PACK_SAMPLES samples (gaps included) or $SDK_DIARIZE_PACK_LINKAGE_BYTES of distance matrices."""
    cap_s = min(MAX_PACK_SAMPLES, max(1, int(os.environ.get("SDK_DIARIZE_PACK_SAMPLES", str(DEFAULT_PACK_SAMPLES)))))
    cap_b = max(1, int(os.environ.get("SDK_DIARIZE_PACK_LINKAGE_BYTES", str(DEFAULT_PACK_LINKAGE_BYTES))))
    packs, cur, ns, nb = [], [], 0, 0
    for i, (size, Cn) in enumerate(zip(sizes, n_chunks)):
        s_i, b_i = size + CHUNK, 8 * (N_LOCAL * Cn) ** 2
        if s_i > MAX_PACK_SAMPLES:
            raise ValueError(f"diarize_many: recording {i}: {size} samples; a pack holds fewer than 2^31 with its gap")
        if cur and (ns + s_i > cap_s or nb + b_i > cap_b):
            packs.append(cur)
            cur, ns, nb = [], 0, 0
        cur.append(i)
        ns, nb = ns + s_i, nb + b_i
    if cur:
        packs.append(cur)
    return packs


def _dot_in_order(A: np.ndarray, B: np.ndarray) -> np.ndarray:
    """A [m, d], B [K, d] float64 -> [m, K]: every entry one sum over the columns in ascending order (the kernels' order; numpy's own
    reductions add pairwise)."""
    acc = np.zeros((A.shape[0], B.shape[0]))
    for j in range(A.shape[1]):
        acc += A[:, j, None] * B[None, :, j]
    return acc


def assign_grouped_host(E, info, cent64, chunk_off, cent_off, constrained: bool = False):
    """sdk_diarize_assign_grouped in numpy: E [3 C, d], info [C, 3, 4], cent64 [K, d] float64, chunk_off / cent_off [R + 1] ->
    (labels [C, 3] int32 local to the recording, score [C, 3] float64).  Rows that are no candidates are never read."""
    ok = candidate_mask(info).reshape(-1, N_LOCAL)
    Cn = ok.shape[0]
    labels, score = np.full((Cn, N_LOCAL), -1, np.int32), np.zeros((Cn, N_LOCAL))
    cent64 = np.asarray(cent64, dtype=np.float64)
    for r in range(len(chunk_off) - 1):
        cent = cent64[int(cent_off[r]):int(cent_off[r + 1])]
        if not cent.shape[0]:
            continue
        for c in range(int(chunk_off[r]), int(chunk_off[r + 1])):
            slots = np.flatnonzero(ok[c])
            if not slots.size:
                continue
            cos = _dot_in_order(np.asarray(E)[c * N_LOCAL + slots].astype(np.float64), cent)
            if constrained:
                lab = constrained_chunk(cos)
            else:
                lab = [int(np.argmax(np.where(row == row, row, -np.inf))) if (row == row).any() else -1 for row in cos]   # a NaN never wins
            for s, row, k in zip(slots, cos, lab):
                if k >= 0:
                    labels[c, s], score[c, s] = k, row[k]
    return labels, score


def fold_grouped_host(cent64, sizes, cl_off, eff, cent_off) -> np.ndarray:
    """sdk_diarize_fold_grouped in numpy: the cut's unit centroids [Kc, d] float64, sizes [Kc], cl_off [R + 1], eff [R], cent_off [R + 1] ->
    remap [Kc] int32, the final global cluster (cent_off[r] + number by first appearance) of every cluster of the cut."""
    cent64, sizes = np.asarray(cent64, dtype=np.float64), np.asarray(sizes)
    remap = np.full(sizes.shape[0], -1, np.int32)
    for r in range(len(cl_off) - 1):
        b, e = int(cl_off[r]), int(cl_off[r + 1])
        if b == e:
            continue
        large = b + np.flatnonzero(sizes[b:e] >= eff[r])
        target = np.arange(b, e)
        if large.size == 0:
            target[:] = b
        else:
            small = b + np.flatnonzero(sizes[b:e] < eff[r])
            if small.size:
                cos = _dot_in_order(cent64[small], cent64[large])
                cos = np.where(cos == cos, cos, -np.inf)                  # a NaN never wins; all NaN: the first large cluster
                target[small - b] = large[np.argmax(cos, axis=1)]         # first maximum: the lower cluster
        _, first = np.unique(target, return_index=True)                   # kept clusters by the lowest cluster sent to them
        new = {int(t): int(cent_off[r]) + n for n, t in enumerate(target[np.sort(first)])}
        remap[b:e] = [new[int(t)] for t in target]
    return remap


def reconstruct_grouped_host(cls, starts_local, labels, chunk_off, frame_off, n_samples, cent_off, max_speakers: Optional[int] = None):
    """sdk_diarize_reconstruct_grouped in numpy -> (count [G] uint8, speakers [G, 2] int32, act: one [G_r, max(K_r, 1)] int32 table per
    recording) on the packed frame grid."""
    G = int(frame_off[-1])
    count, speakers, acts = np.zeros(G, np.uint8), np.full((G, 2), -1, np.int32), []
    for r in range(len(chunk_off) - 1):
        a, b = int(chunk_off[r]), int(chunk_off[r + 1])
        K = max(int(cent_off[r + 1] - cent_off[r]), 1)
        n_g = int(frame_off[r + 1] - frame_off[r])
        if a == b or n_g == 0:
            acts.append(np.zeros((n_g, K), np.int32))
            continue
        cnt, spk, act, _ = reconstruct_host(np.asarray(cls)[a:b], np.asarray(starts_local)[a:b], np.asarray(labels)[a:b], K, int(n_samples[r]), max_speakers)
        g0 = int(frame_off[r])
        m = min(n_g, len(cnt))
        count[g0:g0 + m], speakers[g0:g0 + m] = cnt[:m], spk[:m]
        acts.append(act)
    return count, speakers, acts


def first_seen_host(speakers, frame_off, cent_off) -> np.ndarray:
    """sdk_diarize_first_seen in numpy -> first [K] int32: the least 2 g + slot (g inside the recording) at which the cluster stands in
    speakers [G, 2] of its recording, INT32_MAX when never."""
    sp = np.asarray(speakers).reshape(-1, 2)
    first = np.full(int(cent_off[-1]), np.iinfo(np.int32).max, np.int32)
    for r in range(len(frame_off) - 1):
        flat = sp[int(frame_off[r]):int(frame_off[r + 1])].reshape(-1)
        pos = np.flatnonzero((flat >= 0) & (flat < cent_off[r + 1] - cent_off[r]))
        np.minimum.at(first, int(cent_off[r]) + flat[pos], pos.astype(np.int32))
    return first


def renumber_host(first, cent_off, chunk_off, labels, cent):
    """sdk_diarize_renumber in numpy: renum [K] = rank of (first[k], k) inside the recording (appearance_order); -> (renum, labels
    rewritten, cent rows permuted)."""
    first, labels, cent = np.asarray(first), np.array(labels, dtype=np.int32), np.asarray(cent)
    renum, out = np.zeros(len(first), np.int32), np.empty_like(cent)
    for r in range(len(cent_off) - 1):
        b, e = int(cent_off[r]), int(cent_off[r + 1])
        order = np.lexsort((np.arange(e - b), first[b:e]))                # by first, then by cluster
        renum[b + order] = np.arange(e - b)
        out[b + renum[b:e]] = cent[b:e]
        lab = labels[int(chunk_off[r]):int(chunk_off[r + 1])]
        ok = (lab >= 0) & (lab < e - b)                                   # a label at or above the recording's cluster count stays as it is
        lab[ok] = renum[b + lab[ok]]
    return renum, labels, out


