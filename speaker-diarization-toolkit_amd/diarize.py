"""Speaker diarization - "who spoke when" for a recording with no transcript: the join of the PyanNet segmentation (segmentation.py), the
ResNet34 embedding (resnet.py) and the centroid-linkage clustering (cluster.agglomerative_cluster), as PyAnnote 3.1's pipeline joins them
("Pyannote local speaker diarization" in the upstream toolkit's backends.yaml).  The rules below are THIS build's statement, following
PyAnnote 3.1 as best known here; no checkpoint and no pyannote code is on hand, so PARITY IS UNPINNED, like the three stages joined, and the
tests pin these rules.

  chunks      10-s chunks at segmentation.chunk_starts (step_s apart, plus one ending at the recording's end), cut on the device
  decode      cls [C, F] uint8 = argmax powerset class per frame (ties to the lower class); activity and count come from cls alone
  masks       per (chunk, local speaker s): pooling weights over the T4 columns of the ResNet's last map.  Column j takes segmentation frame
              i(j) = min(F - 1, (j F) // T4); full[j] = s active at i(j); clean[j] = full[j] and count(i(j)) < 2; the weights are clean when
              sum clean >= MIN_CLEAN_COLUMNS, else full; valid = sum w >= MIN_VALID_COLUMNS (the unbiased variance needs two columns)
  embedding   one conv trunk per chunk, three masked statistics poolings on its last map (ResNet34.forward_masked), seg_1, L2 norm.
              PyAnnote embeds each (chunk, speaker) pair with a full forward on the same waveform; the mask enters at the pooling only, so
              sharing the trunk computes the same thing in a third of the work.
  training    rows that are valid and have TRAIN_CLEAN_DEN * clean_frames >= F go to cluster.agglomerative_cluster unchanged
  assignment  centroids = float64 mean of each cluster's training unit rows, re-normalised; every valid row with an active frame takes the
              centroid of largest cosine (ties to the lowest); every other pair gets -1.  No training row: one cluster of all valid active
              rows (centroid = their mean), or no speaker at all.
  constrained assignment (constrained=True; PyAnnote's constrained_argmax): same centroids, same candidates (the local speakers of a chunk
              with valid != 0 and active frames > 0, in slot order; every other pair gets -1 and its row is never read).  For a chunk with m
              candidates and K centroids: among all maps that give n = min(m, K) of the candidates pairwise different clusters and the
              other m - n candidates -1, the one with the largest total cosine, summed in slot order; ties to the lexicographically smallest
              label tuple in slot order, -1 ordered after every cluster.  Two local speakers of a chunk - two different people, says the
              segmentation - never share a cluster.  A candidate left without a cluster (K < m) is DROPPED, as in PyAnnote: when the
              clustering finds one speaker, overlapped speech of a second one is lost.  With K >= m the optimum uses, for every row, one
              of that row's m largest cosines (ties to the lower cluster), so at most 27 tuples are compared per chunk and no general
              Hungarian solver is needed.  Runs on the device (sdk_diarize_centroids, sdk_diarize_assign): the embeddings stay there.
  VBx         (clustering="vbx"; the clustering half of PyAnnote's speaker-diarization-community-1 pipeline, stated in cluster.vbx_cluster):
              the centroid linkage of the training rows, cut at `threshold` with no small-cluster fold, only INITIALISES a variational-Bayes
              mixture on the PLDA transform of those rows (plda.py); speakers that the cut over-split lose their weight and die out.  The
              kept speakers' centroids are the responsibility-weighted means of the original unit rows; every candidate row is then assigned
              by sdk_diarize_assign with the caller's `constrained` flag, so the stretch from embeddings to labels stays on the device and the
              result carries scores either way.  With fewer than two training rows: as "ahc" (one cluster or none).
  bounds      (speakers=; pyannote's num_speakers / min_speakers / max_speakers, written from the published description; parity unpinned, the
              tests pin THIS rule, stated in full in cluster.py above parse_speakers).  None: no bound, every result field is what it was.
              An int k >= 1: exactly k speakers; a pair (lo, hi), either side None, 1 <= lo <= hi: bounds; pyannote's max_speakers is
              speakers=(None, hi) here, while max_speakers below stays the cap PER FRAME and never touches the clustering.  The
              unbounded clustering runs first and finds K0 speakers ("ahc": the clusters after cut and fold; "vbx": the kept speakers).
              lo <= K0 <= hi: the result IS the unbounded one, bit for bit.  Otherwise target = lo when K0 < lo, else hi, clamped to
              1 .. N training rows.  "ahc": the level search of cluster.agglomerative_cluster rule 7 (host integers on Z, O(N)): the level
              whose count of clusters of the effective minimum size is nearest the target, then nearest the cut, then lowest, folded as
              the cut is; a target above K0 may be out of reach, then the closest count is taken.  "vbx": cluster.kmeans_cluster with
              k = target on the original unit rows of the training set (sdk_kmeans_rows: the whole loop in one enqueue), whose labels go
              through sdk_diarize_centroids and sdk_diarize_assign as VBx's centroids do; pi and elbo of the VBx pass that was overruled
              stay on the result.  With fewer than two training rows nothing is forced.  The result's `forced` is None, or
              {found: K0, target, method: "level" | "kmeans", level: t* or None, n_iter: int or None}.  In run_many the level search
              replaces the cut per recording inside _pack_ahc, on the host: the waits per pack do not grow.
  stitching   on the global frame grid of segmentation.aggregate_counts (frame g, centre 270 g + 495, takes frame g + q_c of chunk c,
              q_c = (135 - start_c) // 270): act[g, k] = chunks in which a local speaker labelled k is active; count[g] = the mean chunk count
              rounded half up, at most 2 and max_speakers; speakers[g] = the count[g] clusters of largest act > 0 (ties to the lower cluster)
  numbering   clusters are renumbered by first appearance in time: frame order, then slot order, of a provisional stitching pass (clusters
              that never surface keep their relative order behind the others); the stitching is then run with the final numbers
  turns       per speaker, runs of frames with segmentation.frames_to_ranges's boundaries; no gap filling; overlap gives simultaneous turns

  many        (Diarizer.run_many, Backend.diarize_many) a folder of recordings crosses the pipeline as packs: the recordings laid end to end in
              one buffer with CHUNK zero samples behind each (pack_recordings), so chunks of different recordings share the segmentation /
              embedding batches and a chunk that runs past its recording's end reads zeros, as it does alone; ONE grouped centroid_linkage
              launch for all recordings; the cut per recording on the host (integers and Z); fold, centroids, assignment, stitching and the
              renumbering by appearance in grouped kernels (sdk_diarize_*_grouped, sdk_diarize_first_seen, sdk_diarize_renumber) that find
              a chunk's, frame's or cluster's recording by binary search on prefix-sum tables.  The embeddings never leave the device and
              the host waits for the device a fixed number of times per pack.
  linking     (link_speakers, Backend.link_speakers) the speakers of many recordings as one inventory: the results' centroids, grouped by
              recording, go through the linked centroid linkage on the device (cluster.link_rows, sdk_linked_linkage: two speakers of one
              recording never join, merging stops at the threshold); enrolled profiles join as rows of one further group.  The rule is
              stated at link_speakers; run_many's results are not changed by it.
  streaming   (Diarizer.open_streams, Backend.open_streams) audio fed as it arrives, "who is speaking now" a bounded delay later: the same chunks
              and embed_chunks, then an inventory that grows online, the constrained assignment above against its centroids and a rolling
              stitch on this frame grid that emits frames once their latency has passed.  The rule, its numpy restatement and the bank of
              live streams that steps in one launch are stream.py's; run and run_many are not changed by it.
  score       (Diarizer.score, Backend.score_diarization) how good a result is: the diarization error rate of results against reference
              annotations (turn lists, or RTTM), on this frame grid.  The results' speakers tables are scored on the device as one pack -
              reference masks, co-occurrence tallies and the exact reference-to-hypothesis assignment in three integer kernels
              (csrc/score.hip).  The rule, its numpy restatement (score_host) and the RTTM reader are score.py's.
  sweep       (Diarizer.sweep, Backend.tune_diarization) the DER of run_many at many thresholds, for tuning the cut on a development set:
              per pack one embedding and one linkage (_pack_link), then per threshold the cut-to-centroids stage (_pack_cut), the grouped
              assignment and stitching, and the scoring kernels on the hypothesis where it lies; every threshold's tallies come down in one
              download per pack.  clustering="ahc" without speaker bounds only; run_many is not changed by it.
  shared      run and run_many are one pipeline: Diarizer._check_options, _check_recording, _embed_all (the batches of embed_chunks) and
              _empty serve both, as do candidate_mask, training_mask and _speaker_cap; after the embedding run clusters one recording and
              run_many takes the pack through _pack_rows, _pack_vbx or _pack_ahc, _pack_assign and _pack_results.  They differ on purpose in
              two places, both for "ahc": run(constrained=False) assigns on the host (assign_rows, a BLAS product, no scores) and run folds
              small clusters on the host (cluster.agglomerative_cluster, a BLAS product), where run_many's grouped kernels sum every cosine
              in column order in float64 (every result carries scores).  So with constrained=True run_many's cls, info, labels, count,
              speakers, turns, n_speakers and starts equal run's, and with constrained=False too unless a decision is a tie or near-tie at
              float64 rounding; centroids agree to fp32 rounding of the same float64 rows.

Decode, masks, the constrained assignment and stitching run in libsdk_hip.so (csrc/diarize.hip), the pooling in csrc/resnet.hip; the *_host
functions below restate them in numpy for hosts that post-process stored class tables.  The host receives info, the unit embeddings (not
with constrained=True: then labels, scores and centroids instead), and count / speakers only.
"""
from __future__ import annotations

import os
import time
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from .cluster import PYANNOTE_MIN_CLUSTER_SIZE, PYANNOTE_THRESHOLD
from .segmentation import CHUNK, FRAME_HOP, POWERSET, SAMPLE_RATE, chunk_starts, frames_to_ranges
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
    forced = None                             # speakers= overruled the clustering: {found, target, method, level, n_iter} ("bounds" above); else None


# ------------------------------------------------------------------------------------------------ host restatements (numpy, vectorised)
def global_frames(n_samples: int) -> int:
    return max(0, (int(n_samples) - 495 + FRAME_HOP - 1) // FRAME_HOP)


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
        for k in {int(v) for v in labels[c] if v >= 0}:
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


def assign_rows(E: np.ndarray, info: np.ndarray, train: np.ndarray, train_labels: np.ndarray):
    """Unit rows E [C * 3, d], info, the training rows and their cluster labels -> (labels [C, 3] int32, centroids [K, d] fp32 unit)."""
    E64 = np.asarray(E, dtype=np.float64)
    ok = candidate_mask(info)
    cand = np.flatnonzero(ok)
    labels = np.full(ok.size, -1, np.int32)
    if len(train):
        K = int(np.max(train_labels)) + 1
        cent = np.zeros((K, E64.shape[1]))
        np.add.at(cent, np.asarray(train_labels, dtype=np.int64), E64[train])
        cent /= np.bincount(train_labels, minlength=K)[:, None]
    elif len(cand):
        cent = E64[cand].mean(0, keepdims=True)
    else:
        return labels.reshape(-1, N_LOCAL), np.zeros((0, E64.shape[1]), np.float32)
    cent /= np.maximum(np.linalg.norm(cent, axis=1, keepdims=True), 1e-300)
    if len(cand):
        labels[cand] = np.argmax(E64[cand] @ cent.T, axis=1)              # first maximum: ties to the lowest centroid
    return labels.reshape(-1, N_LOCAL), cent.astype(np.float32)


def _centroids64(E64: np.ndarray, cand: np.ndarray, train: np.ndarray, train_labels: np.ndarray) -> np.ndarray:
    """The float64 unit centroids of assign_rows ([0, d] when there is neither a training row nor a candidate)."""
    if len(train):
        K = int(np.max(train_labels)) + 1
        cent = np.zeros((K, E64.shape[1]))
        np.add.at(cent, np.asarray(train_labels, dtype=np.int64), E64[train])
        cent /= np.bincount(train_labels, minlength=K)[:, None]
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


# ------------------------------------------------------------------------------------------------ speakers across recordings
@dataclass
class SpeakerLinks:
    ids: List[np.ndarray]                     # per recording, int32 [K_r]: the global speaker of every local speaker
    n_global: int
    centroids: np.ndarray                     # [n_global, d] unit fp32: float64 mean of the member unit centroids, re-normalised (profiles excluded)
    profile: np.ndarray                       # [n_global] int32: the row of `profiles` in the speaker's cluster, else -1
    linkage: np.ndarray                       # the merges made over the offered rows (cluster.LinkResult.linkage)
    n_merges: int
    names: Optional[list] = None              # Backend.link_speakers with candidates: [n_global] speaker_id or None


def link_speakers(eng, results, threshold: float = PYANNOTE_THRESHOLD, min_speech_s: float = 0.0, profiles=None) -> SpeakerLinks:
    """One speaker inventory for a list of DiarizationResult (Diarizer.run_many's, in order): which local speakers of different recordings are
    the same person.  Parity with any outside tool is unpinned; the tests pin this rule.

      rows       the `centroids` of every result, in recording order then local speaker order; the group of a row is its recording's index, so
                 two speakers of one recording - two different people, say the segmentation and the clustering - never share a global speaker
      min_speech_s  a local speaker whose turns total less than this many seconds is not offered to the linkage: it stays a speaker of its own
      profiles   [P, d] unit fp32, one row per enrolled speaker, appended after all recording rows with the one group R (the number of
                 recordings): no cluster ever holds two enrolled speakers
      linkage    cluster.link_rows (the linked centroid linkage on the device, csrc/ahc.hip) with stop = threshold
      numbering  global speakers are numbered by first appearance, in recording order then local speaker number; a cluster that holds only a
                 profile gets no id
      centroids  of a global speaker: the float64 mean of its members' unit centroids, re-normalised, stored fp32; a profile row is no member

    The default threshold is PyAnnote 3.1's WITHIN-recording value for single embeddings: it is untuned for centroids across recordings
    (averaged rows lie closer together than single ones do); pass a threshold chosen on your own data."""
    from .cluster import link_rows
    import torch
    R = len(results)
    cents = [np.asarray(res.centroids, dtype=np.float32) for res in results]
    for r, c in enumerate(cents):
        if c.ndim != 2:
            raise ValueError(f"link_speakers: recording {r}: centroids must be [K, d], got {list(c.shape)}")
    prof = None if profiles is None else np.ascontiguousarray(profiles, dtype=np.float32)
    if prof is not None and prof.ndim != 2:
        raise ValueError(f"link_speakers: profiles must be [P, d], got {list(prof.shape)}")
    dims = {c.shape[1] for c in cents if c.shape[0]} | ({prof.shape[1]} if prof is not None and prof.shape[0] else set())
    if len(dims) > 1:
        raise ValueError(f"link_speakers: centroids and profiles of different widths {sorted(dims)}: one embedding space is needed")
    d = dims.pop() if dims else 0
    if not float(min_speech_s) >= 0.0:
        raise ValueError(f"link_speakers: min_speech_s={min_speech_s} (seconds, >= 0)")
    owner = [(r, k) for r in range(R) for k in range(cents[r].shape[0])]            # every local speaker, in numbering order
    offered = []
    for r, k in owner:
        total = sum(b - a for a, b, s in results[r].turns if s == k)
        offered.append(total >= float(min_speech_s))
    P = 0 if prof is None else int(prof.shape[0])
    rows = [cents[r][k] for (r, k), on in zip(owner, offered) if on] + [prof[p] for p in range(P)]
    group = [r for (r, _), on in zip(owner, offered) if on] + [R] * P
    n_rec = len(rows) - P
    if rows:
        E = torch.from_numpy(np.ascontiguousarray(np.stack(rows), dtype=np.float32))
        dev = getattr(eng, "device", None)
        link = link_rows(eng, E if dev is None else E.to(dev), np.asarray(group, np.int32), threshold)
    else:
        link = link_rows(eng, np.zeros((0, d), np.float32), np.zeros(0, np.int32), threshold)
    prof_of = {int(link.labels[n_rec + p]): p for p in range(P)}                    # cluster -> its profile row (at most one: they share a group)
    ids = [np.zeros(c.shape[0], np.int32) for c in cents]
    gid_of, members, profile = {}, [], []
    j = 0
    for (r, k), on in zip(owner, offered):
        c = None
        if on:
            c, j = int(link.labels[j]), j + 1
        if c is None or c not in gid_of:
            if c is not None:
                gid_of[c] = len(members)
            ids[r][k] = len(members)
            members.append([(r, k)])
            profile.append(prof_of.get(c, -1) if c is not None else -1)
        else:
            ids[r][k] = gid_of[c]
            members[gid_of[c]].append((r, k))
    out = np.zeros((len(members), d), np.float32)
    for gidx, m in enumerate(members):
        mean = np.stack([cents[r][k] for r, k in m]).astype(np.float64).mean(axis=0)
        out[gidx] = (mean / max(float(np.linalg.norm(mean)), 1e-12)).astype(np.float32)
    return SpeakerLinks(ids, len(members), out, np.asarray(profile, np.int32).reshape(-1), link.linkage, link.n_merges)


def relabel_turns(result, ids_r) -> List[Tuple[float, float, int]]:
    """A recording's turns with its local speakers replaced by their global ones (SpeakerLinks.ids[r]), by start then speaker."""
    ids_r = np.asarray(ids_r)
    return sorted(((a, b, int(ids_r[k])) for a, b, k in result.turns), key=lambda t: (t[0], t[2]))


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
                target[small - b] = large[np.argmax(_dot_in_order(cent64[small], cent64[large]), axis=1)]   # first maximum: the lower cluster
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
        lab[lab >= 0] = renum[b + lab[lab >= 0]]
    return renum, labels, out


# ------------------------------------------------------------------------------------------------ device stages
VBX_HOST_READS = 7               # cluster.vbx_cluster waits for the device 7 times: the linkage's status and Z, the one read (n_iter, status, K), labels, pi, elbo, keep
LINKAGE_HOST_READS = 1           # Engine.centroid_linkage reads its status back before it returns Z


def _native():
    """(torch, _lib.check, ops._stream), imported at the first call and not with this module: the host restatements need neither."""
    import torch
    from ._lib import check
    from .ops import _stream
    return torch, check, _stream


def _check_dim(name: str, d: int):
    if d < 64 or d % 64 or d > MAX_ASSIGN_DIM:
        raise ValueError(f"{name}: d={d} not supported (a multiple of 64, at most {MAX_ASSIGN_DIM})")


def _check_rows(name: str, E, rows: Optional[int] = None):
    if E.dim() != 2 or str(E.dtype) != "torch.float32" or not E.is_contiguous() or not E.is_cuda or (rows is not None and E.shape[0] != rows):
        raise ValueError(f"{name}: E must be a contiguous fp32 [{'rows' if rows is None else rows}, d] device tensor, got {tuple(E.shape)} {E.dtype}")
    _check_dim(name, int(E.shape[1]))


def _check_tensor(name: str, what: str, t, dtype: str, shape: tuple, min_rows: int = 0):
    """The wrappers' check of cls (uint8 [C, F]), labels (int32 [C, 3]), info (int32 [C, 3, 4]), the centroids (float64 [K, d]) and the like:
    contiguous, torch's dtype `dtype`, of `shape` (None: any size), at least min_rows rows."""
    if str(t.dtype) != "torch." + dtype or t.dim() != len(shape) or any(n not in (None, m) for n, m in zip(shape, t.shape)) or not t.is_contiguous() or t.shape[0] < min_rows:
        raise ValueError(f"{name}: {what} must be a contiguous {dtype} tensor of shape {shape} (None: any size; {min_rows} rows or more), got {tuple(t.shape)} {t.dtype}")


def powerset_decode(eng, logp):
    """logp [C, F, 7] fp32 (device) -> cls [C, F] uint8 (device): sdk_powerset_decode."""
    torch, check, _stream = _native()
    logp = logp.contiguous()
    _check_tensor("powerset_decode", "logp", logp, "float32", (None, None, 7))
    cls = torch.empty(logp.shape[:2], dtype=torch.uint8, device=logp.device)
    check(eng.lib.sdk_powerset_decode(eng.ctx, logp.data_ptr(), logp.shape[0], logp.shape[1], cls.data_ptr(), _stream()), "sdk_powerset_decode")
    return cls


def diarize_masks(eng, cls, T4: int):
    """cls [B, F] uint8 (device) -> (w [B, 3, T4] fp32, info [B, 3, 4] int32) on the device: sdk_diarize_masks."""
    torch, check, _stream = _native()
    _check_tensor("diarize_masks", "cls", cls, "uint8", (None, None))
    B, F = cls.shape
    w = torch.empty((B, N_LOCAL, T4), dtype=torch.float32, device=cls.device)
    info = torch.empty((B, N_LOCAL, 4), dtype=torch.int32, device=cls.device)
    check(eng.lib.sdk_diarize_masks(eng.ctx, cls.data_ptr(), B, F, int(T4), w.data_ptr(), info.data_ptr(), _stream()), "sdk_diarize_masks")
    return w, info


def diarize_reconstruct(eng, cls, starts, labels, K: int, n_samples: int, max_speakers: Optional[int] = None, want_act: bool = False):
    """cls [C, F] uint8, starts [C] int32 ascending, labels [C, 3] int32 (all on the device) -> (count [G] uint8, speakers [G, 2] int32,
    act [G, K] int32 or None) on the device: sdk_diarize_reconstruct."""
    torch, check, _stream = _native()
    _check_tensor("diarize_reconstruct", "cls", cls, "uint8", (None, None))
    Cn, F = cls.shape
    starts, labels = starts.contiguous(), labels.contiguous()
    _check_tensor("diarize_reconstruct", "starts", starts, "int32", (Cn,))
    _check_tensor("diarize_reconstruct", "labels", labels, "int32", (Cn, N_LOCAL))
    G = int(eng.lib.sdk_diarize_frames(int(n_samples)))
    count = torch.zeros((G,), dtype=torch.uint8, device=cls.device)
    speakers = torch.full((G, 2), -1, dtype=torch.int32, device=cls.device)
    act = torch.zeros((G, int(K)), dtype=torch.int32, device=cls.device) if want_act else None
    check(eng.lib.sdk_diarize_reconstruct(eng.ctx, cls.data_ptr(), starts.data_ptr(), labels.data_ptr(), Cn, F, int(K), int(n_samples),
                                          _speaker_cap(max_speakers), count.data_ptr(), speakers.data_ptr(), act.data_ptr() if want_act else None,
                                          _stream()), "sdk_diarize_reconstruct")
    return count, speakers, act


def diarize_centroids(eng, E, rows, labels, K: int, check_rows: bool = True):
    """E [R, d] fp32 unit rows, rows [n] int32 ascending, labels [n] int32 in [0, K) (all on the device) -> (cent [K, d] fp32 unit,
    cent64 [K, d] float64) on the device: sdk_diarize_centroids.  A cluster without rows gives a zero row.  check_rows=False: the caller
    has checked that rows lie in [0, R) (the check reads them back, which waits for the device)."""
    torch, check, _stream = _native()
    _check_rows("diarize_centroids", E)
    if int(K) < 1:
        raise ValueError(f"diarize_centroids: K={K} (at least 1)")
    rows, labels = rows.contiguous(), labels.contiguous()
    _check_tensor("diarize_centroids", "rows", rows, "int32", (None,))
    _check_tensor("diarize_centroids", "labels", labels, "int32", tuple(rows.shape))
    n, d = int(rows.numel()), int(E.shape[1])
    if check_rows and n and not (0 <= int(rows.min()) and int(rows.max()) < E.shape[0]):   # the kernel reads E at these rows
        raise ValueError(f"diarize_centroids: rows must lie in [0, {E.shape[0]}), got {int(rows.min())} .. {int(rows.max())}")
    cent = torch.empty((int(K), d), dtype=torch.float32, device=E.device)
    cent64 = torch.empty((int(K), d), dtype=torch.float64, device=E.device)
    check(eng.lib.sdk_diarize_centroids(eng.ctx, E.data_ptr(), rows.data_ptr(), labels.data_ptr(), n, int(K), d, cent.data_ptr(), cent64.data_ptr(),
                                        _stream()), "sdk_diarize_centroids")
    return cent, cent64


def diarize_assign(eng, E, info, cent, constrained: bool = False):
    """E [3 C, d] fp32 unit rows, info [C, 3, 4] int32, cent [K, d] float64 (diarize_centroids' second result), all on the device ->
    (labels [C, 3] int32, score [C, 3] fp32) on the device: sdk_diarize_assign."""
    torch, check, _stream = _native()
    Cn = E.shape[0] // N_LOCAL
    _check_rows("diarize_assign", E, N_LOCAL * Cn)
    d = int(E.shape[1])
    _check_tensor("diarize_assign", "info", info, "int32", (Cn, N_LOCAL, 4))
    _check_tensor("diarize_assign", "the centroids", cent, "float64", (None, d))
    if cent.shape[0] < 1:
        raise ValueError("diarize_assign: K=0 (at least one centroid)")
    labels = torch.empty((Cn, N_LOCAL), dtype=torch.int32, device=E.device)
    score = torch.empty((Cn, N_LOCAL), dtype=torch.float32, device=E.device)
    check(eng.lib.sdk_diarize_assign(eng.ctx, E.data_ptr(), info.data_ptr(), cent.data_ptr(), Cn, int(cent.shape[0]), d, int(bool(constrained)),
                                     labels.data_ptr(), score.data_ptr(), _stream()), "sdk_diarize_assign")
    return labels, score


class GroupTables:
    """The prefix-sum tables of a pack on the host (checked here, once) and on the device (what the grouped kernels search).  uploads counts
    the host-to-device copies made so far."""

    def __init__(self, eng, chunk_off, frame_off, n_samples, starts_local=None):
        self.eng, self.uploads = eng, 0
        self.chunk_off, self.frame_off = np.asarray(chunk_off, dtype=np.int64), np.asarray(frame_off, dtype=np.int64)
        self.n_samples = np.asarray(n_samples, dtype=np.int64)
        self.R = R = int(self.n_samples.size)
        for name, off in (("chunk_off", self.chunk_off), ("frame_off", self.frame_off)):
            if R < 1 or off.shape != (R + 1,) or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] >= (1 << 30):
                raise ValueError(f"GroupTables: {name} must hold R + 1 = {R + 1} prefix sums from 0 (below 2^30), got {off.tolist()[:8]}")
        if not np.array_equal(np.diff(self.frame_off), [global_frames(int(n)) for n in self.n_samples]):
            raise ValueError("GroupTables: frame_off must be the prefix sums of global_frames(n_samples)")
        self.C, self.G = int(self.chunk_off[-1]), int(self.frame_off[-1])
        parts = [self.chunk_off, self.frame_off] + ([np.asarray(starts_local, dtype=np.int64)] if starts_local is not None else [])
        if starts_local is not None and parts[2].shape != (self.C,):
            raise ValueError(f"GroupTables: starts_local must hold {self.C} chunk starts, got {parts[2].shape}")
        up = self._up(np.concatenate(parts).astype(np.int32))                                        # one upload
        self.chunk_off_d, self.frame_off_d = up[:R + 1], up[R + 1:2 * R + 2]
        self.starts_local_d = up[2 * R + 2:] if starts_local is not None else None
        self.n_samples_d = self._up(self.n_samples)
        self.cent_off = self.cent_off_d = self.act_off = self.act_off_d = None
        self.K = 0

    def _up(self, a: np.ndarray):
        self.uploads += 1
        return _native()[0].from_numpy(a).to(self.eng.device)

    def set_clusters(self, cent_off, want_act: bool = False):
        """cent_off [R + 1]: prefix sums of the recordings' cluster counts."""
        off = np.asarray(cent_off, dtype=np.int64)
        if off.shape != (self.R + 1,) or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] >= (1 << 30):
            raise ValueError(f"GroupTables: cent_off must hold R + 1 = {self.R + 1} prefix sums from 0, got {off.tolist()[:8]}")
        self.cent_off, self.K = off, int(off[-1])
        self.cent_off_d = self._up(off.astype(np.int32))
        self.act_off = np.concatenate([[0], np.cumsum(np.diff(self.frame_off) * np.maximum(np.diff(off), 1))]).astype(np.int64)
        self.act_off_d = self._up(self.act_off) if want_act else None
        return self


def diarize_assign_grouped(eng, E, info, cent, tab: GroupTables, constrained: bool = False):
    """diarize_assign over a pack: cent [K, d] float64 holds recording r's centroids at tab.cent_off[r] .. tab.cent_off[r + 1] ->
    (labels [C, 3] int32 local to the recording, score [C, 3] fp32) on the device: sdk_diarize_assign_grouped."""
    torch, check, _stream = _native()
    _check_rows("diarize_assign_grouped", E, N_LOCAL * tab.C)
    Cn, d = tab.C, int(E.shape[1])
    _check_tensor("diarize_assign_grouped", "info", info, "int32", (Cn, N_LOCAL, 4))
    if tab.cent_off is None:
        raise ValueError("diarize_assign_grouped: the tables hold no clusters (set_clusters)")
    _check_tensor("diarize_assign_grouped", "the centroids", cent, "float64", (None, d), max(tab.K, 1))
    labels = torch.empty((Cn, N_LOCAL), dtype=torch.int32, device=E.device)
    score = torch.empty((Cn, N_LOCAL), dtype=torch.float32, device=E.device)
    check(eng.lib.sdk_diarize_assign_grouped(eng.ctx, E.data_ptr(), info.data_ptr(), cent.data_ptr(), tab.chunk_off_d.data_ptr(), tab.cent_off_d.data_ptr(),
                                             tab.R, Cn, d, int(bool(constrained)), labels.data_ptr(), score.data_ptr(), _stream()), "sdk_diarize_assign_grouped")
    return labels, score


def diarize_fold_grouped(eng, cent, sizes, cl_off, eff, cent_off, cut=None, upload=None):
    """The fold of cluster.fold_small_clusters over a pack, on the device: cent [Kc, d] float64 unit centroids of the cut (device), sizes
    [Kc], cl_off [R + 1], eff [R], cent_off [R + 1] (host integers; cent_off must count the large clusters of every recording, 1 when it has
    clusters and none is large), cut [n] int32 (device, or None): the cut's global cluster of every training row ->
    (remap [Kc] int32, out [n] int32 = remap[cut], or None) on the device: sdk_diarize_fold_grouped.  upload: what carries the one table of
    host integers to cent's device (a caller that counts its transfers passes its own)."""
    torch, check, _stream = _native()
    sizes, cl_off, eff, cent_off = (np.asarray(v, dtype=np.int64) for v in (sizes, cl_off, eff, cent_off))
    R, Kc = int(eff.size), int(sizes.size)
    large = None
    if R >= 1 and cl_off.shape == (R + 1,) and cl_off[0] == 0 and cl_off[-1] == Kc and (np.diff(cl_off) >= 0).all():
        rec = np.repeat(np.arange(R), np.diff(cl_off))                    # the recording of every cluster of the cut
        large = np.bincount(rec[sizes >= eff[rec]], minlength=R)
    if large is None or cent_off.shape != (R + 1,) or cent_off[0] != 0 or not np.array_equal(np.diff(cent_off), np.where(np.diff(cl_off) > 0, np.maximum(large, 1), 0)):
        raise ValueError("diarize_fold_grouped: cl_off must be the R + 1 prefix sums of the cut's cluster counts and cent_off those of the large clusters (1 when none)")
    _check_tensor("diarize_fold_grouped", "the centroids", cent, "float64", (None, None), Kc)
    d = int(cent.shape[1])
    _check_dim("diarize_fold_grouped", d)
    n = 0 if cut is None else int(cut.numel())
    if cut is not None:
        _check_tensor("diarize_fold_grouped", "cut", cut, "int32", (None,))
    up = (upload or (lambda a: torch.from_numpy(a).to(cent.device)))(np.concatenate([sizes, cl_off, eff, cent_off]).astype(np.int32))
    sizes_d, cl_d, eff_d, co_d = up[:Kc], up[Kc:Kc + R + 1], up[Kc + R + 1:Kc + 2 * R + 1], up[Kc + 2 * R + 1:]
    target = torch.empty((max(Kc, 1),), dtype=torch.int32, device=cent.device)
    remap = torch.empty((max(Kc, 1),), dtype=torch.int32, device=cent.device)
    out = torch.empty((max(n, 1),), dtype=torch.int32, device=cent.device)
    check(eng.lib.sdk_diarize_fold_grouped(eng.ctx, cent.data_ptr(), sizes_d.data_ptr(), cl_d.data_ptr(), eff_d.data_ptr(), co_d.data_ptr(), R, Kc, d,
                                           target.data_ptr(), remap.data_ptr(), cut.data_ptr() if n else None, n, out.data_ptr(), _stream()),
          "sdk_diarize_fold_grouped")
    return remap[:Kc], (out[:n] if cut is not None else None)


def diarize_reconstruct_grouped(eng, cls, labels, tab: GroupTables, max_speakers: Optional[int] = None, want_act: bool = False):
    """diarize_reconstruct over a pack: cls [C, F] uint8, labels [C, 3] int32 local to the recording (device), tab with starts_local and
    clusters set -> (count [G] uint8, speakers [G, 2] int32, act int32 [tab.act_off[-1]] or None) on the packed frame grid:
    sdk_diarize_reconstruct_grouped."""
    torch, check, _stream = _native()
    _check_tensor("diarize_reconstruct_grouped", "cls", cls, "uint8", (tab.C, None))
    _check_tensor("diarize_reconstruct_grouped", "labels", labels, "int32", (tab.C, N_LOCAL))
    if tab.starts_local_d is None or tab.cent_off is None or (want_act and tab.act_off_d is None):
        raise ValueError("diarize_reconstruct_grouped: the tables need starts_local and set_clusters (want_act=True for act)")
    count = torch.zeros((tab.G,), dtype=torch.uint8, device=cls.device)
    speakers = torch.full((tab.G, 2), -1, dtype=torch.int32, device=cls.device)
    act = torch.zeros((max(int(tab.act_off[-1]), 1),), dtype=torch.int32, device=cls.device) if want_act else None
    if tab.C and tab.G:
        check(eng.lib.sdk_diarize_reconstruct_grouped(eng.ctx, cls.data_ptr(), tab.starts_local_d.data_ptr(), labels.data_ptr(), tab.chunk_off_d.data_ptr(),
                                                      tab.frame_off_d.data_ptr(), tab.n_samples_d.data_ptr(), tab.cent_off_d.data_ptr(), tab.R, tab.C,
                                                      int(cls.shape[1]), tab.G, _speaker_cap(max_speakers), count.data_ptr(), speakers.data_ptr(),
                                                      act.data_ptr() if want_act else None, tab.act_off_d.data_ptr() if want_act else None, _stream()),
              "sdk_diarize_reconstruct_grouped")
    return count, speakers, act


def diarize_first_seen(eng, speakers, tab: GroupTables):
    """speakers [G, 2] int32 (device) -> first [K] int32 (device): sdk_diarize_first_seen (integer atomicMin)."""
    torch, check, _stream = _native()
    if speakers.dtype != torch.int32 or tuple(speakers.shape) != (tab.G, 2) or not speakers.is_contiguous() or tab.cent_off is None:
        raise ValueError(f"diarize_first_seen: speakers must be a contiguous int32 [{tab.G}, 2] tensor and the tables hold clusters, got {tuple(speakers.shape)} {speakers.dtype}")
    first = torch.empty((max(tab.K, 1),), dtype=torch.int32, device=speakers.device)
    check(eng.lib.sdk_diarize_first_seen(eng.ctx, speakers.data_ptr(), tab.frame_off_d.data_ptr(), tab.cent_off_d.data_ptr(), tab.R, tab.G, tab.K,
                                         first.data_ptr(), _stream()), "sdk_diarize_first_seen")
    return first[:tab.K]


def diarize_renumber(eng, first, labels, cent, cent64, tab: GroupTables):
    """first [K] (diarize_first_seen), labels [C, 3] int32 local (REWRITTEN in place), cent [K, d] fp32 and cent64 [K, d] float64 ->
    (renum [K] int32, cent and cent64 with recording r's rows permuted to their new numbers) on the device: sdk_diarize_renumber."""
    torch, check, _stream = _native()
    K = tab.K
    _check_tensor("diarize_renumber", "first", first, "int32", (K,))
    _check_tensor("diarize_renumber", "labels", labels, "int32", (tab.C, N_LOCAL))
    _check_tensor("diarize_renumber", "cent64", cent64, "float64", (None, None), K)
    _check_tensor("diarize_renumber", "cent", cent, "float32", tuple(cent64.shape))
    renum = torch.empty((max(K, 1),), dtype=torch.int32, device=labels.device)
    o32, o64 = torch.empty_like(cent), torch.empty_like(cent64)
    check(eng.lib.sdk_diarize_renumber(eng.ctx, first.data_ptr(), tab.cent_off_d.data_ptr(), tab.chunk_off_d.data_ptr(), tab.R, K, tab.C, int(cent.shape[1]),
                                       renum.data_ptr(), labels.data_ptr(), cent.data_ptr(), cent64.data_ptr(), o32.data_ptr(), o64.data_ptr(), _stream()),
          "sdk_diarize_renumber")
    return renum[:K], o32, o64


class Diarizer:
    """The pipeline on one ops.Engine: a resident segmentation.Segmentation and a resident embedding network - resnet.ResNet34, or
    ecapa_diar.EcapaEmbedder for a diarization in the ECAPA space; any object with .cfg.embed_dim, .precision, .last_map_frames(T) and
    .forward_masked(feats, B, T, w, valid) serves (the parameter and the attribute keep the name `resnet`; `embedder` is its read-only
    alias).  run and run_many share the option
    and recording checks, the embedding of all chunks (_embed_all) and the empty result; they part after that (the module docstring)."""

    def __init__(self, engine, segmentation, resnet, plda=None):
        self.eng, self.seg, self.resnet, self.plda = engine, segmentation, resnet, plda
        self.trace = False               # True: run_many appends one {stage: seconds} per pack to last_stage_s, every stage ended by a device synchronisation
        self.last_stage_s: List[dict] = []
        self.last_sync: List[dict] = []  # run_many: the downloads and uploads of the last call, one dict per pack

    @property
    def embedder(self):
        """The embedding network (read-only; the attribute `resnet` under its family-neutral name).  Any object with .cfg.embed_dim,
        .precision, .last_map_frames(T) and .forward_masked(feats, B, T, w, valid) serves: resnet.ResNet34, or ecapa_diar.EcapaEmbedder."""
        return self.resnet

    def plda_model(self):
        """The plda.Plda of clustering="vbx": the one given, else a seeded synthetic model for the embedding width."""
        if self.plda is None:
            from .plda import synthetic_plda
            self.plda = synthetic_plda(self.resnet.cfg.embed_dim, 128, 0)
        return self.plda

    # ---------------------------------------------------------------------------------------------- what run and run_many share
    def _check_options(self, who: str, clustering, vbx, max_speakers, speakers=None):
        """-> (vbx as a dict of its own, the bounds of cluster.parse_speakers)."""
        if clustering not in ("ahc", "vbx"):
            raise ValueError(f"{who}: clustering={clustering!r} (\"ahc\" or \"vbx\")")
        vbx = dict(vbx or {})
        if set(vbx) - {"Fa", "Fb", "max_iters", "epsilon", "init_smoothing"} or (vbx and clustering != "vbx"):
            raise ValueError(f"{who}: vbx={vbx} (keys Fa, Fb, max_iters, epsilon, init_smoothing; only with clustering=\"vbx\")")
        if max_speakers is not None and int(max_speakers) < 0:
            raise ValueError(f"max_speakers={max_speakers}: must be None or >= 0")
        from .cluster import parse_speakers
        return vbx, parse_speakers(speakers, who)

    def _check_recording(self, who: str, Cn: int, n_samples: int, step_s: float, logp=None):
        """The linkage's row bound and the shape of an injected logp, for a recording of n_samples > 0 samples in Cn chunks."""
        F = seg_frames(CHUNK)
        if N_LOCAL * Cn > MAX_LINKAGE_ROWS:
            raise ValueError(f"{who}: {Cn} chunks at step_s={step_s} give up to {N_LOCAL * Cn} embeddings to cluster; the centroid linkage serves at "
                             f"most {MAX_LINKAGE_ROWS} rows ({MAX_LINKAGE_ROWS // N_LOCAL} chunks): raise step_s or split the recording")
        if logp is not None:
            shp = tuple(logp.shape if hasattr(logp, "shape") else np.shape(logp))
            if shp != (Cn, F, 7):
                raise ValueError(f"{who}: injected logp must be [{Cn}, {F}, 7] for {n_samples} samples at step_s={step_s}, got {shp}")

    def _empty(self) -> DiarizationResult:
        d = self.resnet.cfg.embed_dim
        return DiarizationResult([], 0, np.zeros((0, d), np.float32), np.zeros((0, N_LOCAL), np.int32), np.zeros(0, np.uint8),
                                 np.full((0, 2), -1, np.int32), np.zeros(0, np.int64), np.zeros((0, N_LOCAL, 4), np.int32))

    def embed_chunks(self, rec, n_samples: int, starts_dev, logp=None):
        """One batch of chunks: (cls [B, F] uint8, info [B, 3, 4] int32, unit embeddings [B * 3, d] fp32), all on the device."""
        from .ops import num_frames as fbank_frames
        B = int(starts_dev.numel())
        lp = logp if logp is not None else self.seg.forward(rec, starts_dev)
        cls = powerset_decode(self.eng, lp)
        T = fbank_frames(CHUNK)
        w, info = diarize_masks(self.eng, cls, self.resnet.last_map_frames(T))
        feats = self.eng.fbank_windows(rec.data_ptr(), n_samples, starts_dev.data_ptr(), B, CHUNK)
        emb = self.resnet.forward_masked(feats, B, T, w, info[:, :, 3].contiguous())
        return cls, info, self.eng.l2norm(emb)[0]

    def _embed_all(self, rec, n: int, starts_dev, logp_dev=None):
        """Every chunk of the buffer rec (n samples, device) in batches of $SDK_DIARIZE_BATCH -> (cls [C, F] uint8, info [C, 3, 4] int32,
        unit embeddings [3 C, d] fp32) on the device.  In a pack the batches cross recording boundaries."""
        torch = _native()[0]
        Cn = int(starts_dev.numel())
        batch = max(1, int(os.environ.get("SDK_DIARIZE_BATCH", str(DEFAULT_BATCH))))
        cls = torch.empty((Cn, seg_frames(CHUNK)), dtype=torch.uint8, device=self.eng.device)
        infos, embs = [], []
        for a in range(0, Cn, batch):
            c, i, e = self.embed_chunks(rec, n, starts_dev[a:a + batch], None if logp_dev is None else logp_dev[a:a + batch])
            cls[a:a + batch] = c
            infos.append(i)
            embs.append(e)
        return cls, torch.cat(infos), torch.cat(embs)

    def open_streams(self, n_streams: int = 1, **options):
        """A stream.StreamBank of n_streams live streams on this pipeline (options: step_s, latency_s, capacity, delta_new, max_speakers;
        stream.py states the rule)."""
        from .stream import StreamBank
        return StreamBank(self, n_streams, **options)

    # ---------------------------------------------------------------------------------------------- one recording
    def run(self, samples, step_s: float = 1.0, threshold: float = PYANNOTE_THRESHOLD, min_cluster_size: int = PYANNOTE_MIN_CLUSTER_SIZE,
            max_speakers: Optional[int] = None, logp=None, constrained: bool = False, clustering: str = "ahc",
            vbx: Optional[dict] = None, speakers=None) -> DiarizationResult:
        """samples: 16 kHz mono int16 (host) -> DiarizationResult.  logp [C, 589, 7] (fp32, host or device) replaces the segmentation
        model's output (the chunks are chunk_starts(len(samples), step_s)).  The default threshold and size are PyAnnote 3.1's, tuned for
        ITS trained embedding; with other weights pass a threshold of your own.  constrained=True: the constrained assignment of the
        module docstring, on the device (the result carries scores); False: every row takes its nearest centroid on its own.
        clustering="vbx": the VBx clustering of the module docstring instead of the cut-and-fold ("ahc", the default); `threshold` keeps its
        meaning, the cut of the linkage, which now only initialises: pass cluster.VBX_AHC_THRESHOLD (0.6) with it; min_cluster_size is not
        used.  vbx: a dict of Fa, Fb, max_iters, epsilon, init_smoothing (cluster.vbx_cluster's defaults otherwise).  The result carries
        scores, pi and elbo.
        speakers: the number of speakers of the recording, "bounds" in the module docstring: None, an int k (exactly k) or a pair (lo, hi),
        either side None.  pyannote's num_speakers=k is speakers=k, its min_speakers / max_speakers are speakers=(lo, hi), its
        max_speakers alone is speakers=(None, hi); max_speakers HERE is the cap per frame and keeps that meaning.  The result's `forced`
        says whether the clustering was overruled."""
        vbx, bounds = self._check_options("diarize", clustering, vbx, max_speakers, speakers)
        torch = _native()[0]
        from .cluster import agglomerative_cluster, vbx_cluster
        eng = self.eng
        x = np.ascontiguousarray(samples, dtype=np.int16).reshape(-1)
        if x.size == 0:
            return self._empty()
        st = chunk_starts(x.size, step_s)                       # chunks
        Cn, F = len(st), seg_frames(CHUNK)
        self._check_recording("diarize", Cn, x.size, step_s, logp)
        if logp is not None:
            logp = torch.as_tensor(logp, dtype=torch.float32).to(eng.device)
        if eng.precision != self.resnet.precision:
            eng.set_precision(self.resnet.precision)            # the front end's output format follows the embedding's numerical contract
        rec = torch.from_numpy(x).to(eng.device)
        starts_dev = torch.from_numpy(st.astype(np.int32)).to(eng.device)
        cls, info_dev, E_dev = self._embed_all(rec, x.size, starts_dev, logp)     # decode, masks, embedding
        info = info_dev.cpu().numpy()
        train = training_rows(info, F)                          # training rows and their clustering
        vres, tl, forced = None, np.zeros(len(train), np.int32), None
        if len(train) > 1 and clustering == "vbx":
            vres = vbx_cluster(eng, E_dev, self.plda_model(), threshold, rows=train, speakers=bounds, **vbx)
            forced = vres.forced
        elif len(train) > 1:
            ares = agglomerative_cluster(eng, E_dev.index_select(0, torch.from_numpy(train).to(eng.device)).contiguous(), threshold, min_cluster_size,
                                         speakers=bounds)
            tl, forced = ares.labels, ares.forced
        if constrained or clustering == "vbx":                  # assignment on the device: the embeddings stay there, the result carries scores
            if vres is not None:
                c32, c64 = vres.cent, vres.cent64.contiguous()
            else:
                rows = train if len(train) else np.flatnonzero(candidate_mask(info))                 # no training row: the candidates, one cluster
                rl = np.asarray(tl, dtype=np.int32) if len(train) else np.zeros(len(rows), np.int32)
                c32, c64 = diarize_centroids(eng, E_dev, torch.from_numpy(rows.astype(np.int32)).to(eng.device), torch.from_numpy(rl).to(eng.device),
                                             int(rl.max()) + 1) if len(rows) else (None, None)
            if c64 is not None:
                lab_dev, score_dev = diarize_assign(eng, E_dev, info_dev, c64, bool(constrained))
                labels, scores, cent = lab_dev.cpu().numpy(), score_dev.cpu().numpy(), c32.cpu().numpy()
            else:                                               # neither a training row nor a candidate: no speaker
                labels, scores, cent = np.full((Cn, N_LOCAL), -1, np.int32), np.zeros((Cn, N_LOCAL), np.float32), np.zeros((0, self.resnet.cfg.embed_dim), np.float32)
        else:                                                   # assignment of "ahc" unconstrained: on the host, a BLAS product (the module docstring)
            E = E_dev.cpu().numpy()
            E[info.reshape(-1, 4)[:, 3] == 0] = 0.0            # rows that are not valid are never read as embeddings
            labels, cent = assign_rows(E, info, train, tl)
            scores = None
        K = cent.shape[0]

        def stitch(lab):                                        # stitching; numbering by appearance below, then turns
            cnt, spk, _ = diarize_reconstruct(eng, cls, starts_dev, torch.from_numpy(np.ascontiguousarray(lab, dtype=np.int32)).to(eng.device),
                                              max(K, 1), x.size, max_speakers)
            return cnt.cpu().numpy(), spk.cpu().numpy()
        count, speakers = stitch(labels)
        if K > 1:
            new = appearance_order(speakers, K)
            if not np.array_equal(new, np.arange(K)):
                labels = np.where(labels >= 0, new[np.maximum(labels, 0)], -1).astype(np.int32)
                cent = cent[np.argsort(new)]
                count, speakers = stitch(labels)
        res = DiarizationResult(turns_from_frames(speakers, K), K, cent, labels, count, speakers, st, info, cls, scores)
        if vres is not None:
            res.pi, res.elbo = vres.pi, vres.elbo
        if forced is not None:
            res.forced = forced
        return res

    # ---------------------------------------------------------------------------------------------- many recordings in one device pass
    def run_many(self, recordings, step_s: float = 1.0, threshold: float = PYANNOTE_THRESHOLD, min_cluster_size: int = PYANNOTE_MIN_CLUSTER_SIZE,
                 max_speakers: Optional[int] = None, logp=None, constrained: bool = False, clustering: str = "ahc",
                 vbx: Optional[dict] = None, speakers=None) -> List[DiarizationResult]:
        """recordings: a list of 16 kHz mono int16 arrays (host) -> one DiarizationResult per recording, in order; the keywords are run's,
        logp is None or a list with one [C_r, 589, 7] array per recording.  The recordings cross the pipeline in packs (pack_recordings) of
        at most $SDK_DIARIZE_PACK_SAMPLES samples (default 2^28, gaps included) whose grouped linkage stays within
        $SDK_DIARIZE_PACK_LINKAGE_BYTES of distance matrices (default 2^34; Engine.centroid_linkage serves any number of problems of at
        most 65 536 rows each); a recording that exceeds either bound alone is a pack of its own.  Per pack: one upload, the batches of
        $SDK_DIARIZE_BATCH chunks (they cross recording boundaries), one download of info, one grouped linkage launch over the recordings
        with at least two training rows and the download of its status and Z, the cut per recording on the host, then centroids of the cut,
        fold, final centroids, assignment, stitching, renumbering and second stitching on the device, and one download each of labels,
        scores, centroids, count and speakers.  self.last_sync holds the number of such waits of the last call, per pack.
        Where the results differ from run's on purpose: "shared" in the module docstring.  clustering="vbx" runs cluster.vbx_cluster
        recording by recording (its own linkage, cut and host reads) between the packed embedding and the grouped assignment.
        speakers: run's, applied to every recording; for "ahc" the level search replaces the cut on the host and adds no wait, for "vbx" a
        recording whose count is overruled adds cluster.KMEANS_HOST_READS waits."""
        from .cluster import vbx_cluster  # noqa: F401  (checked early: the package imports)
        vbx, bounds = self._check_options("diarize_many", clustering, vbx, max_speakers, speakers)
        xs, packs = self._plan_packs(recordings, logp, step_s)
        out: List[Optional[DiarizationResult]] = [None] * len(xs)
        self.last_sync = []
        for idx in packs:
            for i, res in zip(idx, self._run_pack([xs[i] for i in idx], None if logp is None else [logp[i] for i in idx], step_s, threshold,
                                                  min_cluster_size, max_speakers, constrained, clustering, vbx, bounds)):
                out[i] = res
        return out

    def _plan_packs(self, recordings, logp, step_s):
        """run_many's and sweep's checks of the recordings and their split into packs -> (xs as int16 rows, [[recording index]] per pack)."""
        xs = [np.ascontiguousarray(x, dtype=np.int16).reshape(-1) for x in recordings]
        if logp is not None and (not isinstance(logp, (list, tuple)) or len(logp) != len(xs)):
            raise ValueError(f"diarize_many: logp must be None or a list with one array per recording ({len(xs)}), got "
                             f"{len(logp) if isinstance(logp, (list, tuple)) else type(logp).__name__}")
        n_chunks = [len(chunk_starts(x.size, step_s)) if x.size else 0 for x in xs]
        for i, x in enumerate(xs):
            if x.size:
                self._check_recording(f"diarize_many: recording {i}", n_chunks[i], x.size, step_s, None if logp is None else logp[i])
        cap_s = min(MAX_PACK_SAMPLES, max(1, int(os.environ.get("SDK_DIARIZE_PACK_SAMPLES", str(DEFAULT_PACK_SAMPLES)))))
        cap_b = max(1, int(os.environ.get("SDK_DIARIZE_PACK_LINKAGE_BYTES", str(DEFAULT_PACK_LINKAGE_BYTES))))
        packs, cur, ns, nb = [], [], 0, 0
        for i, x in enumerate(xs):
            s_i, b_i = x.size + CHUNK, 8 * (N_LOCAL * n_chunks[i]) ** 2
            if s_i > MAX_PACK_SAMPLES:
                raise ValueError(f"diarize_many: recording {i}: {x.size} samples; a pack holds fewer than 2^31 with its gap")
            if cur and (ns + s_i > cap_s or nb + b_i > cap_b):
                packs.append(cur)
                cur, ns, nb = [], 0, 0
            cur.append(i)
            ns, nb = ns + s_i, nb + b_i
        if cur:
            packs.append(cur)
        return xs, packs

    # ---------------------------------------------------------------------------------------------- scoring against a reference, threshold sweep
    def score(self, results, references, collar_s: float = 0.0, skip_overlap: bool = False):
        """DiarizationResults (run's, run_many's or a finished stream's) and one reference turn list [(start_s, end_s, name)] per result ->
        one score.DerResult per result: their `speakers` are uploaded and scored on the device as one pack (score.py states the rule)."""
        from .score import MAX_SCORE_SPEAKERS, score_grouped
        results, references = list(results), list(references)
        if len(references) != len(results):
            raise ValueError(f"score: {len(references)} references for {len(results)} recordings")
        if not results:
            return []
        spk = [np.ascontiguousarray(res.speakers, dtype=np.int32).reshape(-1, 2) for res in results]
        for r, (res, sp) in enumerate(zip(results, spk)):
            if sp.size and int(sp.max()) >= int(res.n_speakers):
                raise ValueError(f"score: recording {r}: speakers names {int(sp.max())}, the result has {res.n_speakers} speakers")
            if int(res.n_speakers) > MAX_SCORE_SPEAKERS:
                raise ValueError(f"score: recording {r}: {res.n_speakers} hypothesis speakers; at most {MAX_SCORE_SPEAKERS} per recording")
        torch = _native()[0]
        G_r = [len(sp) for sp in spk]
        n_samples = [FRAME_HOP * g + 226 if g else 0 for g in G_r]                      # a length with global_frames(n) == g: only the grid is read
        tab = GroupTables(self.eng, np.zeros(len(results) + 1, np.int64), np.concatenate([[0], np.cumsum(G_r)]), n_samples)
        tab.set_clusters(np.concatenate([[0], np.cumsum([int(res.n_speakers) for res in results])]))
        spk_dev = torch.from_numpy(np.concatenate(spk)).to(self.eng.device)
        return score_grouped(self.eng, spk_dev, tab, references, collar_s, skip_overlap)

    def sweep(self, recordings, references, thresholds, step_s: float = 1.0, min_cluster_size: int = PYANNOTE_MIN_CLUSTER_SIZE,
              max_speakers: Optional[int] = None, logp=None, constrained: bool = False, collar_s: float = 0.0, skip_overlap: bool = False,
              clustering: str = "ahc", speakers=None):
        """The DER of run_many(recordings, threshold=t, ...) against `references` for every t of `thresholds` -> score.SweepResult
        (thresholds, per_recording [T][R], pooled [T], best).  Per pack the recordings are embedded ONCE and linked ONCE (_pack_embed,
        _pack_link); per threshold only the cheap tail runs - cut on host integers, fold, centroids, assignment, stitching, renumbering and
        second stitching exactly as run_many's (_pack_cut, _pack_assign_dev), then the three scoring kernels on the hypothesis where it
        lies.  The tallies of all thresholds stay on the device and come down in one download per pack: the waits per pack (last_sync) do
        not grow with the number of thresholds.  Only clustering="ahc" without speaker bounds: the sweep is over the cut of the linkage.
        A recording that the cut splits into more than score.MAX_SCORE_SPEAKERS speakers at some threshold is a ValueError."""
        from .score import SweepResult, best_threshold, pool, rasterise_references, results_from_tables, score_host, score_tables, split_tables
        if clustering != "ahc" or speakers is not None:
            raise ValueError(f"sweep: clustering={clustering!r}, speakers={speakers!r}: the sweep is over the cut of clustering=\"ahc\" with speakers=None")
        self._check_options("sweep", clustering, None, max_speakers, None)
        ths = [float(t) for t in thresholds]
        if not ths or any(t != t for t in ths):
            raise ValueError(f"sweep: thresholds={list(thresholds)!r} (at least one number)")
        references = list(references)
        if len(references) != len(recordings):
            raise ValueError(f"sweep: {len(references)} references for {len(recordings)} recordings")
        xs, packs = self._plan_packs(recordings, logp, step_s)
        per = [[None] * len(xs) for _ in ths]
        self.last_sync = []
        for idx in packs:
            sync = {"downloads": 0, "uploads": 0}
            self.last_sync.append(sync)
            if self.trace:
                self.last_stage_s.append({})
            self._t_mark = time.perf_counter()
            pxs, refs = [xs[i] for i in idx], [references[i] for i in idx]
            pack = pack_recordings(pxs, step_s)
            if int(pack.chunk_off[-1]) == 0:                      # nothing but empty recordings: no frame to score
                for t in range(len(ths)):
                    for i, ref in zip(idx, refs):
                        per[t][i] = score_host(np.zeros((0, 2), np.int32), 0, ref, collar_s, skip_overlap)
                continue
            torch = _native()[0]
            tab, cls, info_dev, E_dev = self._pack_embed(pack, pxs, None if logp is None else [logp[i] for i in idx])
            info = self._down(info_dev)
            self._mark("segmentation_embedding")
            rows, n_train = self._pack_rows(info, pack.chunk_off)
            linkage = self._pack_link(E_dev, rows, n_train)
            ref = rasterise_references(self.eng, tab, refs, collar_s, skip_overlap, upload=self._up)
            self._mark("reference")
            held, shapes = [], []
            for t in ths:
                c32, c64, cent_off, _, _ = self._pack_cut(E_dev, rows, n_train, linkage, t, min_cluster_size, None)
                tab.set_clusters(cent_off)
                self._mark("cut_fold_centroids")
                spk_dev = self._pack_assign_dev(tab, cls, info_dev, E_dev, c32, c64, constrained, max_speakers)[4]
                self._mark("assign_stitch")
                tally, correct, mapping, co, co_off = score_tables(self.eng, spk_dev, tab, ref, upload=self._up)
                held += [tally.reshape(-1), correct, mapping.to(torch.int64), co.to(torch.int64)]
                shapes.append((cent_off, co_off))
                self._mark("score")
            sync["uploads"] += tab.uploads
            flat = self._down(torch.cat(held))                    # every threshold's tallies, tables and maps: ONE download
            pos = 0
            for t, (cent_off, co_off) in enumerate(shapes):
                n = 6 * tab.R + int(ref.ref_off[-1]) + int(co_off[-1])
                res = results_from_tables(ref, cent_off, co_off, *split_tables(flat[pos:pos + n], tab.R, int(ref.ref_off[-1]), int(co_off[-1])))
                pos += n
                for i, one in zip(idx, res):
                    per[t][i] = one
            self._mark("download")
        pooled = [pool(row) for row in per]
        return SweepResult(ths, per, pooled, best_threshold(ths, pooled))

    def _up(self, a, dtype=None):                              # host -> device, counted for the current pack (dtype: torch.as_tensor converts on the way)
        torch = _native()[0]
        self.last_sync[-1]["uploads"] += 1
        return (torch.from_numpy(np.ascontiguousarray(a)) if dtype is None else torch.as_tensor(a, dtype=dtype)).to(self.eng.device)

    def _down(self, t) -> np.ndarray:                           # device -> host, a wait for the device, counted for the current pack
        self.last_sync[-1]["downloads"] += 1
        return t.cpu().numpy()

    def _mark(self, name: str):
        """self.trace: the wall clock since the last mark goes to stage `name` of the current pack, after a device synchronisation."""
        if self.trace:
            _native()[0].cuda.synchronize()
            now, stage_s = time.perf_counter(), self.last_stage_s[-1]
            stage_s[name] = stage_s.get(name, 0.0) + now - self._t_mark
            self._t_mark = now

    def _run_pack(self, xs, logps, step_s, threshold, min_cluster_size, max_speakers, constrained, clustering, vbx, bounds=None):
        """One pack through its stages; every _mark ends a stage of last_stage_s."""
        sync = {"downloads": 0, "uploads": 0}
        self.last_sync.append(sync)
        if self.trace:
            self.last_stage_s.append({})
        self._t_mark = time.perf_counter()
        pack = pack_recordings(xs, step_s)
        if int(pack.chunk_off[-1]) == 0:
            return [self._empty() for _ in xs]
        tab, cls, info_dev, E_dev = self._pack_embed(pack, xs, logps)
        info = self._down(info_dev)
        self._mark("segmentation_embedding")
        rows, n_train = self._pack_rows(info, pack.chunk_off)
        if clustering == "vbx":
            c32, c64, cent_off, vres, forced = self._pack_vbx(E_dev, pack.chunk_off, rows, n_train, threshold, vbx, bounds)
        else:
            c32, c64, cent_off, vres, forced = self._pack_ahc(E_dev, rows, n_train, threshold, min_cluster_size, bounds)
        tab.set_clusters(cent_off)
        sync["uploads"] += tab.uploads
        self._mark("cut_fold_centroids")
        host = self._pack_assign(tab, cls, info_dev, E_dev, c32, c64, constrained, max_speakers)
        self._mark("assign_stitch_download")
        out = self._pack_results(xs, pack, cent_off, info, cls, vres, forced, *host)
        self._mark("turns")
        return out

    def _pack_embed(self, pack: Pack, xs, logps):
        """Upload the pack and its tables, then embed every chunk -> (tab, cls, info_dev, E_dev)."""
        torch = _native()[0]
        if self.eng.precision != self.resnet.precision:
            self.eng.set_precision(self.resnet.precision)       # the front end's output format follows the embedding's numerical contract
        rec = self._up(pack.samples)
        starts_dev = self._up(pack.starts_packed)
        tab = GroupTables(self.eng, pack.chunk_off, pack.frame_off, pack.n_samples, pack.starts_local)
        lp_all = None
        if logps is not None:
            lp_all = torch.cat([self._up(l, torch.float32) for l, x in zip(logps, xs) if x.size])
        self._mark("pack_upload")
        return (tab,) + self._embed_all(rec, int(rec.numel()), starts_dev, lp_all)

    def _pack_rows(self, info: np.ndarray, co: np.ndarray):
        """Per recording: the rows that make its centroids (global rows of E, ascending) and how many of them are training rows."""
        cand_ok, train_ok = candidate_mask(info), training_mask(info, seg_frames(CHUNK))
        rows, n_train = [], []
        for r in range(len(co) - 1):
            a, b = N_LOCAL * int(co[r]), N_LOCAL * int(co[r + 1])
            tr = a + np.flatnonzero(train_ok[a:b])
            n_train.append(len(tr))
            rows.append(tr if len(tr) else a + np.flatnonzero(cand_ok[a:b]))      # no training row: one cluster of the candidates
        return rows, n_train

    def _pack_vbx(self, E_dev, co, rows, n_train, threshold, vbx, bounds=None):
        """cluster.vbx_cluster recording by recording (its own linkage, cut and host reads) -> (c32, c64, cent_off, {recording: VbxResult},
        {recording: forced})."""
        torch = _native()[0]
        from .cluster import KMEANS_HOST_READS, vbx_cluster
        vres, cents, K_r, forced = {}, [], [], {}
        for r in range(len(rows)):
            a, K = N_LOCAL * int(co[r]), min(len(rows[r]), 1)
            if n_train[r] > 1:
                v = vres[r] = vbx_cluster(self.eng, E_dev[a:N_LOCAL * int(co[r + 1])], self.plda_model(), threshold, rows=rows[r] - a, speakers=bounds, **vbx)
                self.last_sync[-1]["downloads"] += VBX_HOST_READS
                if v.forced is not None:
                    forced[r] = v.forced
                    self.last_sync[-1]["downloads"] += KMEANS_HOST_READS
                cents.append((v.cent, v.cent64))
                K = int(v.n_speakers)
            elif K:                                             # one training row, or the candidates: one cluster
                cents.append(diarize_centroids(self.eng, E_dev, self._up(rows[r].astype(np.int32)),
                                               torch.zeros(len(rows[r]), dtype=torch.int32, device=self.eng.device), 1, check_rows=False))
            K_r.append(K)
        c32, c64 = (torch.cat(c).contiguous() for c in zip(*cents)) if cents else (None, None)    # None: no recording has a cluster
        return c32, c64, np.concatenate([[0], np.cumsum(K_r)]).astype(np.int64), vres, forced

    def _pack_ahc(self, E_dev, rows, n_train, threshold, min_cluster_size, bounds=None):
        """The linkage stage (_pack_link), then the cut-to-centroids stage (_pack_cut) -> (c32, c64, cent_off, {}, {recording: forced}), as
        _pack_vbx."""
        return self._pack_cut(E_dev, rows, n_train, self._pack_link(E_dev, rows, n_train), threshold, min_cluster_size, bounds)

    def _pack_link(self, E_dev, rows, n_train):
        """ONE grouped linkage over the recordings with at least two training rows -> (those recordings, the prefix sums of their training
        rows, Z on the host); (no recording, None, None) when there is nothing to link.  It does not depend on the threshold: sweep runs it
        once per pack."""
        link = [r for r in range(len(rows)) if n_train[r] > 1]
        if not link:
            return link, None, None
        off = np.concatenate([[0], np.cumsum([n_train[r] for r in link])]).astype(np.int64)
        E_link = E_dev.index_select(0, self._up(np.concatenate([rows[r] for r in link]))).contiguous()
        Z = self._down(self.eng.centroid_linkage(E_link, off))                     # ONE launch for all recordings; reads status, then Z
        self.last_sync[-1]["downloads"] += LINKAGE_HOST_READS
        self._mark("linkage")
        return link, off, Z

    def _pack_cut(self, E_dev, rows, n_train, linkage, threshold, min_cluster_size, bounds=None):
        """The cut per recording on the host (with bounds: the level search of cluster.agglomerative_cluster rule 7 in its place, host
        integers on the same Z), the cut's centroids, the grouped fold and the final centroids -> (c32, c64, cent_off, {},
        {recording: forced}).  linkage: _pack_link's result."""
        from .cluster import _flat_partition, cut_level, effective_min_size, fcluster_distance, level_search, speaker_target
        eng, R = self.eng, len(rows)
        link, off, Z = linkage
        cuts, forced = {}, {}
        if link:
            for g, r in enumerate(link):
                Zr = Z[int(off[g]) - g:int(off[g + 1]) - g - 1]
                cuts[r] = fcluster_distance(Zr, threshold)
                if bounds is not None:                                             # K0 = the clusters the fold will keep: the large ones of the cut, or one
                    eff_r = effective_min_size(min_cluster_size, n_train[r])
                    found = max(1, int((np.bincount(cuts[r]) >= eff_r).sum()))
                    target = speaker_target(found, bounds, n_train[r])
                    if target is not None:
                        level, _ = level_search(Zr, eff_r, cut_level(Zr, threshold), target)
                        cuts[r] = _flat_partition(Zr, n_train[r], level)
                        forced[r] = {"found": found, "target": target, "method": "level", "level": level, "n_iter": None}
        cut_all, sizes, cl_off, eff, cent_off = [], [], [0], [], [0]
        for r in range(R):
            n = len(rows[r])
            cut = cuts[r] if r in cuts else np.zeros(n, np.int32)                  # one training row, or the candidates: one cluster
            sz = np.bincount(cut) if n else np.zeros(0, np.int64)
            m = min(int(min_cluster_size), max(1, round(0.1 * n))) if r in cuts else 1     # cluster.fold_small_clusters, rule 1
            cut_all.append(cut.astype(np.int64) + cl_off[-1])
            sizes.append(sz)
            eff.append(m)
            cl_off.append(cl_off[-1] + len(sz))
            cent_off.append(cent_off[-1] + (max(1, int((sz >= m).sum())) if len(sz) else 0))
        cent_off = np.asarray(cent_off, np.int64)
        if not cl_off[-1]:
            return None, None, cent_off, {}, forced
        rows_d = self._up(np.concatenate(rows).astype(np.int32))
        cut_d = self._up(np.concatenate(cut_all).astype(np.int32))
        _, cut64 = diarize_centroids(eng, E_dev, rows_d, cut_d, cl_off[-1], check_rows=False)
        _, final_d = diarize_fold_grouped(eng, cut64, np.concatenate(sizes), cl_off, eff, cent_off, cut_d, upload=self._up)
        return diarize_centroids(eng, E_dev, rows_d, final_d, int(cent_off[-1]), check_rows=False) + (cent_off, {}, forced)

    def _pack_assign(self, tab, cls, info_dev, E_dev, c32, c64, constrained, max_speakers):
        """Grouped assignment, stitching, renumbering by appearance and second stitching -> (labels, scores, cent, count, speakers) on the host."""
        return tuple(self._down(t) for t in self._pack_assign_dev(tab, cls, info_dev, E_dev, c32, c64, constrained, max_speakers))

    def _pack_assign_dev(self, tab, cls, info_dev, E_dev, c32, c64, constrained, max_speakers):
        """_pack_assign without its downloads: (labels, scores, cent, count, speakers) on the device."""
        torch, eng = _native()[0], self.eng
        if c64 is None:                                          # no cluster anywhere: the kernels still get a row to point at
            d = self.resnet.cfg.embed_dim
            c32, c64 = torch.zeros((1, d), dtype=torch.float32, device=eng.device), torch.zeros((1, d), dtype=torch.float64, device=eng.device)
        lab_dev, score_dev = diarize_assign_grouped(eng, E_dev, info_dev, c64, tab, bool(constrained))
        _, spk_dev, _ = diarize_reconstruct_grouped(eng, cls, lab_dev, tab, max_speakers)
        first = diarize_first_seen(eng, spk_dev, tab)
        _, c32, c64 = diarize_renumber(eng, first, lab_dev, c32, c64, tab)         # ties in the top-2 go to the lower number: stitch again
        cnt_dev, spk_dev, _ = diarize_reconstruct_grouped(eng, cls, lab_dev, tab, max_speakers)
        return lab_dev, score_dev, c32, cnt_dev, spk_dev

    def _pack_results(self, xs, pack: Pack, cent_off, info, cls, vres, forced, labels, scores, cent, count, speakers):
        """The pack's host arrays cut into one DiarizationResult per recording."""
        out = []
        for r, x in enumerate(xs):
            if x.size == 0:
                out.append(self._empty())
                continue
            a, b, g0, g1, k0, k1 = (int(v) for v in (pack.chunk_off[r], pack.chunk_off[r + 1], pack.frame_off[r], pack.frame_off[r + 1], cent_off[r], cent_off[r + 1]))
            res = DiarizationResult(turns_from_frames(speakers[g0:g1], k1 - k0), k1 - k0, cent[k0:k1].copy(), labels[a:b].copy(), count[g0:g1].copy(),
                                    speakers[g0:g1].copy(), pack.starts_local[a:b].astype(np.int64), info[a:b].copy(), cls[a:b], scores[a:b].copy())
            if r in vres:
                res.pi, res.elbo = vres[r].pi, vres[r].elbo
            if r in forced:
                res.forced = forced[r]
            out.append(res)
        return out
