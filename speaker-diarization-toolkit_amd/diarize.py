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
  stitching   on the global frame grid of segmentation.aggregate_counts (frame g, centre 270 g + 495, takes frame g + q_c of chunk c,
              q_c = (135 - start_c) // 270): act[g, k] = chunks in which a local speaker labelled k is active; count[g] = the mean chunk count
              rounded half up, at most 2 and max_speakers; speakers[g] = the count[g] clusters of largest act > 0 (ties to the lower cluster)
  numbering   clusters are renumbered by first appearance in time: frame order, then slot order, of a provisional stitching pass (clusters
              that never surface keep their relative order behind the others); the stitching is then run with the final numbers
  turns       per speaker, runs of frames with segmentation.frames_to_ranges's boundaries; no gap filling; overlap gives simultaneous turns

Decode, masks, the constrained assignment and stitching run in libsdk_hip.so (csrc/diarize.hip), the pooling in csrc/resnet.hip; the *_host
functions below restate them in numpy for hosts that post-process stored class tables.  The host receives info, the unit embeddings (not
with constrained=True: then labels, scores and centroids instead), and count / speakers only.
"""
from __future__ import annotations

import ctypes as C
import os
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
    centroids: np.ndarray                     # [K, embed_dim] unit fp32, in the embedding space of score_windows and enrolled profiles
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


# ------------------------------------------------------------------------------------------------ host restatements (numpy, vectorised)
def global_frames(n_samples: int) -> int:
    return max(0, (int(n_samples) - 495 + FRAME_HOP - 1) // FRAME_HOP)


def decode_host(logp: np.ndarray) -> np.ndarray:
    """logp [..., 7] -> uint8 argmax class (numpy's first maximum: ties to the lower class)."""
    return np.argmax(np.asarray(logp), axis=-1).astype(np.uint8)


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
    cap = 2 if max_speakers is None else min(2, int(max_speakers))
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


def training_rows(info: np.ndarray, F: int) -> np.ndarray:
    """Rows (c * 3 + s) of the clustering's training set: valid and TRAIN_CLEAN_DEN * clean_frames >= F."""
    i = np.asarray(info).reshape(-1, 4)
    return np.flatnonzero((i[:, 3] != 0) & (TRAIN_CLEAN_DEN * i[:, 1].astype(np.int64) >= F))


def assign_rows(E: np.ndarray, info: np.ndarray, train: np.ndarray, train_labels: np.ndarray):
    """Unit rows E [C * 3, d], info, the training rows and their cluster labels -> (labels [C, 3] int32, centroids [K, d] fp32 unit)."""
    i = np.asarray(info).reshape(-1, 4)
    E64 = np.asarray(E, dtype=np.float64)
    cand = np.flatnonzero((i[:, 3] != 0) & (i[:, 0] > 0))
    labels = np.full(i.shape[0], -1, np.int32)
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
    i = np.asarray(info).reshape(-1, 4)
    Cn = i.shape[0] // N_LOCAL
    ok = ((i[:, 3] != 0) & (i[:, 0] > 0)).reshape(Cn, N_LOCAL)
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


# ------------------------------------------------------------------------------------------------ device stages
def powerset_decode(eng, logp):
    """logp [C, F, 7] fp32 (device) -> cls [C, F] uint8 (device): sdk_powerset_decode."""
    import torch
    from ._lib import check
    from .ops import _stream
    if logp.dim() != 3 or logp.shape[2] != 7 or logp.dtype != torch.float32:
        raise ValueError(f"powerset_decode: logp must be fp32 [C, F, 7], got {tuple(logp.shape)} {logp.dtype}")
    logp = logp.contiguous()
    cls = torch.empty(logp.shape[:2], dtype=torch.uint8, device=logp.device)
    check(eng.lib.sdk_powerset_decode(eng.ctx, logp.data_ptr(), logp.shape[0], logp.shape[1], cls.data_ptr(), _stream()), "sdk_powerset_decode")
    return cls


def diarize_masks(eng, cls, T4: int):
    """cls [B, F] uint8 (device) -> (w [B, 3, T4] fp32, info [B, 3, 4] int32) on the device: sdk_diarize_masks."""
    import torch
    from ._lib import check
    from .ops import _stream
    if cls.dim() != 2 or cls.dtype != torch.uint8 or not cls.is_contiguous():
        raise ValueError(f"diarize_masks: cls must be a contiguous uint8 [B, F] tensor, got {tuple(cls.shape)} {cls.dtype}")
    B, F = cls.shape
    w = torch.empty((B, N_LOCAL, T4), dtype=torch.float32, device=cls.device)
    info = torch.empty((B, N_LOCAL, 4), dtype=torch.int32, device=cls.device)
    check(eng.lib.sdk_diarize_masks(eng.ctx, cls.data_ptr(), B, F, int(T4), w.data_ptr(), info.data_ptr(), _stream()), "sdk_diarize_masks")
    return w, info


def diarize_reconstruct(eng, cls, starts, labels, K: int, n_samples: int, max_speakers: Optional[int] = None, want_act: bool = False):
    """cls [C, F] uint8, starts [C] int32 ascending, labels [C, 3] int32 (all on the device) -> (count [G] uint8, speakers [G, 2] int32,
    act [G, K] int32 or None) on the device: sdk_diarize_reconstruct."""
    import torch
    from ._lib import check
    from .ops import _stream
    if cls.dim() != 2 or cls.dtype != torch.uint8 or not cls.is_contiguous():
        raise ValueError(f"diarize_reconstruct: cls must be a contiguous uint8 [C, F] tensor, got {tuple(cls.shape)} {cls.dtype}")
    Cn, F = cls.shape
    if starts.dtype != torch.int32 or tuple(starts.shape) != (Cn,) or labels.dtype != torch.int32 or tuple(labels.shape) != (Cn, N_LOCAL):
        raise ValueError(f"diarize_reconstruct: starts int32 [{Cn}] and labels int32 [{Cn}, 3] expected, got {tuple(starts.shape)} {starts.dtype}, "
                         f"{tuple(labels.shape)} {labels.dtype}")
    starts, labels = starts.contiguous(), labels.contiguous()
    G = int(eng.lib.sdk_diarize_frames(int(n_samples)))
    cap = 2 if max_speakers is None else min(2, int(max_speakers))
    count = torch.zeros((G,), dtype=torch.uint8, device=cls.device)
    speakers = torch.full((G, 2), -1, dtype=torch.int32, device=cls.device)
    act = torch.zeros((G, int(K)), dtype=torch.int32, device=cls.device) if want_act else None
    check(eng.lib.sdk_diarize_reconstruct(eng.ctx, cls.data_ptr(), starts.data_ptr(), labels.data_ptr(), Cn, F, int(K), int(n_samples), cap,
                                          count.data_ptr(), speakers.data_ptr(), act.data_ptr() if want_act else None, _stream()),
          "sdk_diarize_reconstruct")
    return count, speakers, act


def _check_rows(name: str, E, d_what: str = "E"):
    import torch
    if E.dim() != 2 or E.dtype != torch.float32 or not E.is_contiguous() or not E.is_cuda:
        raise ValueError(f"{name}: {d_what} must be a contiguous fp32 [rows, d] device tensor, got {tuple(E.shape)} {E.dtype}")
    if E.shape[1] < 64 or E.shape[1] % 64 or E.shape[1] > MAX_ASSIGN_DIM:
        raise ValueError(f"{name}: d={E.shape[1]} not supported (a multiple of 64, at most {MAX_ASSIGN_DIM})")


def diarize_centroids(eng, E, rows, labels, K: int):
    """E [R, d] fp32 unit rows, rows [n] int32 ascending, labels [n] int32 in [0, K) (all on the device) -> (cent [K, d] fp32 unit,
    cent64 [K, d] float64) on the device: sdk_diarize_centroids.  A cluster without rows gives a zero row."""
    import torch
    from ._lib import check
    from .ops import _stream
    _check_rows("diarize_centroids", E)
    if int(K) < 1:
        raise ValueError(f"diarize_centroids: K={K} (at least 1)")
    if rows.dtype != torch.int32 or labels.dtype != torch.int32 or rows.dim() != 1 or rows.shape != labels.shape:
        raise ValueError(f"diarize_centroids: rows and labels must be int32 [n] tensors of one length, got {tuple(rows.shape)} {rows.dtype}, "
                         f"{tuple(labels.shape)} {labels.dtype}")
    rows, labels = rows.contiguous(), labels.contiguous()
    n, d = int(rows.numel()), int(E.shape[1])
    if n and not (0 <= int(rows.min()) and int(rows.max()) < E.shape[0]):   # the kernel reads E at these rows
        raise ValueError(f"diarize_centroids: rows must lie in [0, {E.shape[0]}), got {int(rows.min())} .. {int(rows.max())}")
    cent = torch.empty((int(K), d), dtype=torch.float32, device=E.device)
    cent64 = torch.empty((int(K), d), dtype=torch.float64, device=E.device)
    check(eng.lib.sdk_diarize_centroids(eng.ctx, E.data_ptr(), rows.data_ptr(), labels.data_ptr(), n, int(K), d, cent.data_ptr(), cent64.data_ptr(),
                                        _stream()), "sdk_diarize_centroids")
    return cent, cent64


def diarize_assign(eng, E, info, cent, constrained: bool = False):
    """E [3 C, d] fp32 unit rows, info [C, 3, 4] int32, cent [K, d] float64 (diarize_centroids' second result), all on the device ->
    (labels [C, 3] int32, score [C, 3] fp32) on the device: sdk_diarize_assign."""
    import torch
    from ._lib import check
    from .ops import _stream
    _check_rows("diarize_assign", E)
    Cn, d = E.shape[0] // N_LOCAL, int(E.shape[1])
    if E.shape[0] % N_LOCAL or info.dtype != torch.int32 or tuple(info.shape) != (Cn, N_LOCAL, 4) or not info.is_contiguous():
        raise ValueError(f"diarize_assign: E [3 C, d] and a contiguous int32 info [C, 3, 4] expected, got {tuple(E.shape)}, {tuple(info.shape)} {info.dtype}")
    if cent.dim() != 2 or cent.dtype != torch.float64 or cent.shape[1] != d or not cent.is_contiguous():
        raise ValueError(f"diarize_assign: the centroids must be a contiguous float64 [K, {d}] tensor, got {tuple(cent.shape)} {cent.dtype}")
    if cent.shape[0] < 1:
        raise ValueError("diarize_assign: K=0 (at least one centroid)")
    labels = torch.empty((Cn, N_LOCAL), dtype=torch.int32, device=E.device)
    score = torch.empty((Cn, N_LOCAL), dtype=torch.float32, device=E.device)
    check(eng.lib.sdk_diarize_assign(eng.ctx, E.data_ptr(), info.data_ptr(), cent.data_ptr(), Cn, int(cent.shape[0]), d, int(bool(constrained)),
                                     labels.data_ptr(), score.data_ptr(), _stream()), "sdk_diarize_assign")
    return labels, score


class Diarizer:
    """The pipeline on one ops.Engine: a resident segmentation.Segmentation and a resident resnet.ResNet34."""

    def __init__(self, engine, segmentation, resnet, plda=None):
        self.eng, self.seg, self.resnet, self.plda = engine, segmentation, resnet, plda

    def plda_model(self):
        """The plda.Plda of clustering="vbx": the one given, else a seeded synthetic model for the embedding width."""
        if self.plda is None:
            from .plda import synthetic_plda
            self.plda = synthetic_plda(self.resnet.cfg.embed_dim, 128, 0)
        return self.plda

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

    def run(self, samples, step_s: float = 1.0, threshold: float = PYANNOTE_THRESHOLD, min_cluster_size: int = PYANNOTE_MIN_CLUSTER_SIZE,
            max_speakers: Optional[int] = None, logp=None, constrained: bool = False, clustering: str = "ahc",
            vbx: Optional[dict] = None) -> DiarizationResult:
        """samples: 16 kHz mono int16 (host) -> DiarizationResult.  logp [C, 589, 7] (fp32, host or device) replaces the segmentation
        model's output (the chunks are chunk_starts(len(samples), step_s)).  The default threshold and size are PyAnnote 3.1's, tuned for
        ITS trained embedding; with other weights pass a threshold of your own.  constrained=True: the constrained assignment of the
        module docstring, on the device (the result carries scores); False: every row takes its nearest centroid on its own.
        clustering="vbx": the VBx clustering of the module docstring instead of the cut-and-fold ("ahc", the default); `threshold` keeps its
        meaning, the cut of the linkage, which now only initialises: pass cluster.VBX_AHC_THRESHOLD (0.6) with it; min_cluster_size is not
        used.  vbx: a dict of Fa, Fb, max_iters, epsilon, init_smoothing (cluster.vbx_cluster's defaults otherwise).  The result carries
        scores, pi and elbo."""
        import torch
        from .cluster import agglomerative_cluster, vbx_cluster
        eng = self.eng
        if clustering not in ("ahc", "vbx"):
            raise ValueError(f"diarize: clustering={clustering!r} (\"ahc\" or \"vbx\")")
        vbx = dict(vbx or {})
        unknown = sorted(set(vbx) - {"Fa", "Fb", "max_iters", "epsilon", "init_smoothing"})
        if unknown or (vbx and clustering != "vbx"):
            raise ValueError(f"diarize: vbx={vbx} (keys Fa, Fb, max_iters, epsilon, init_smoothing; only with clustering=\"vbx\")")
        x = np.ascontiguousarray(samples, dtype=np.int16).reshape(-1)
        d = self.resnet.cfg.embed_dim
        if x.size == 0:
            return DiarizationResult([], 0, np.zeros((0, d), np.float32), np.zeros((0, N_LOCAL), np.int32), np.zeros(0, np.uint8),
                                     np.full((0, 2), -1, np.int32), np.zeros(0, np.int64), np.zeros((0, N_LOCAL, 4), np.int32))
        if max_speakers is not None and int(max_speakers) < 0:
            raise ValueError(f"max_speakers={max_speakers}: must be None or >= 0")
        st = chunk_starts(x.size, step_s)
        Cn, F = len(st), seg_frames(CHUNK)
        if N_LOCAL * Cn > MAX_LINKAGE_ROWS:
            raise ValueError(f"diarize: {Cn} chunks at step_s={step_s} give up to {N_LOCAL * Cn} embeddings to cluster; the centroid linkage serves at "
                             f"most {MAX_LINKAGE_ROWS} rows ({MAX_LINKAGE_ROWS // N_LOCAL} chunks): raise step_s or split the recording")
        if logp is not None:
            logp = torch.as_tensor(logp, dtype=torch.float32).to(eng.device)
            if tuple(logp.shape) != (Cn, F, 7):
                raise ValueError(f"diarize: injected logp must be [{Cn}, {F}, 7] for {x.size} samples at step_s={step_s}, got {tuple(logp.shape)}")
        if eng.precision != self.resnet.precision:
            eng.set_precision(self.resnet.precision)            # the front end's output format follows the embedding's numerical contract
        rec = torch.from_numpy(x).to(eng.device)
        starts_dev = torch.from_numpy(st.astype(np.int32)).to(eng.device)
        batch = max(1, int(os.environ.get("SDK_DIARIZE_BATCH", str(DEFAULT_BATCH))))
        cls = torch.empty((Cn, F), dtype=torch.uint8, device=eng.device)
        infos, embs = [], []
        for a in range(0, Cn, batch):
            c, i, e = self.embed_chunks(rec, x.size, starts_dev[a:a + batch], None if logp is None else logp[a:a + batch])
            cls[a:a + batch] = c
            infos.append(i)
            embs.append(e)
        E_dev = torch.cat(embs)
        info_dev = torch.cat(infos)
        info = info_dev.cpu().numpy()
        train = training_rows(info, F)
        vres = None
        if clustering == "vbx" and len(train) > 1:
            vres = vbx_cluster(eng, E_dev, self.plda_model(), threshold, rows=train, **vbx)
            tl = None
        elif len(train) > 1:
            tl = agglomerative_cluster(eng, E_dev.index_select(0, torch.from_numpy(train).to(eng.device)).contiguous(), threshold, min_cluster_size).labels
        else:
            tl = np.zeros(len(train), np.int32)
        scores = None
        if vres is not None:
            lab_dev, score_dev = diarize_assign(eng, E_dev, info_dev.contiguous(), vres.cent64.contiguous(), bool(constrained))
            labels, scores, cent = lab_dev.cpu().numpy(), score_dev.cpu().numpy(), vres.cent.cpu().numpy()
        elif constrained or clustering == "vbx":
            flat = info.reshape(-1, 4)
            rows, rl = (train, tl) if len(train) else (np.flatnonzero((flat[:, 3] != 0) & (flat[:, 0] > 0)), None)    # no training row: the candidates, one cluster
            if len(rows):
                rl = np.zeros(len(rows), np.int32) if rl is None else np.asarray(rl, dtype=np.int32)
                c32, c64 = diarize_centroids(eng, E_dev, torch.from_numpy(rows.astype(np.int32)).to(eng.device), torch.from_numpy(rl).to(eng.device),
                                             int(rl.max()) + 1)
                lab_dev, score_dev = diarize_assign(eng, E_dev, info_dev.contiguous(), c64, bool(constrained))
                labels, scores, cent = lab_dev.cpu().numpy(), score_dev.cpu().numpy(), c32.cpu().numpy()
            else:
                labels, scores, cent = np.full((Cn, N_LOCAL), -1, np.int32), np.zeros((Cn, N_LOCAL), np.float32), np.zeros((0, d), np.float32)
        else:
            E = E_dev.cpu().numpy()
            E[info.reshape(-1, 4)[:, 3] == 0] = 0.0             # rows that are not valid are never read as embeddings
            labels, cent = assign_rows(E, info, train, tl)
        K = cent.shape[0]

        def stitch(lab):
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
        return res
