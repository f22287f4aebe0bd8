"""Speaker samples: each diarized speaker's cleanest stretches of audio - the clips to listen to and to enrol from - read off the per-frame
speakers of a diarization (diarize.DiarizationResult.speakers) and scored with the identify model (backend.speaker_samples / write_samples,
functions of backend.py).  The rule below is THIS build's statement; no other toolkit's sample picker is on hand (the toolkit's
`speaker_samples extract` works from transcript words, not from frames), so PARITY IS UNPINNED and the tests pin this rule.  Only the two
defaults come from that tool: min_s = 0.5 (--min-duration) and max_gap_s = 1.0 (--max-gap).

  grid        that of score.py / words.py: frame g of a recording has centre sample 270 g + 495 and covers the samples [270 g + 360,
              270 g + 630), g < G = global_frames(n_samples).  The hypothesis is a result's speakers [G, 2] (int32) and its n_speakers = K
  kinds       an entry < 0 or >= K names nobody; a speaker named twice counts once.  Frame g is SILENT when it names nobody, SOLO FOR k
              when the set it names is exactly {k} - (k, -1), (-1, k) and (k, k) - and OVERLAPPED otherwise
  runs        gap = floor(max_gap_s * 16000 + 0.5) // 270 frames (words.gap_frames).  A run of speaker k is a maximal interval [g0, g1)
              inside one recording whose frames g0 and g1 - 1 are solo for k, whose frames are all solo for k or silent, and in which no
              stretch of consecutive silent frames is longer than gap: an overlapped frame, a frame solo for another speaker, gap + 1
              silent frames or the end of the recording end it.  The runs of a recording are pairwise disjoint, listed by ascending g0.
              solo = the solo frames of the run; min_frames = max(1, ceil(floor(min_s * 16000 + 0.5) / 270)); a run is kept iff
              solo >= min_frames.  Row per kept run [4] int32: (speaker, g0, g1, solo), g0 and g1 local to the recording
  limits      at most words.MAX_WORD_SPEAKERS = 1024 speakers per recording: more is a ValueError here and refused by the library
  clips       (host, integers; cut_clips) a run covers the samples s0 = 270 g0 + 360 to s1 = min(270 g1 + 360, n_samples), L = s1 - s0.
              max_clip_s None: the run is one clip.  Else c = floor(max_clip_s * 16000 + 0.5), n = ceil(L / c) and clip i is
              [s0 + floor(i L / n), s0 + floor((i + 1) L / n)); it carries floor(solo / n) of the run's solo frames, the first
              solo mod n clips one more.  max_candidates (None: all): per speaker only the first that many clips in the order (solo
              descending, start ascending) go on to be embedded
  scores      the clips are embedded with Backend.embed_ranges - the identify model, so the scores live in the space of the enrolled
              profiles whatever the diarizer's embedder is; a clip embed_ranges drops (shorter than its least window) is not a sample.
              c_i = the float64 sum of clip i's window rows, m_s = the float64 sum of the c_i of speaker s, cos(a, b) = a . b / (|a| |b|):
              own [i] = cos(c_i, m_s - c_i), the leave-one-out score; 0.0 with alone = 1 when either vector has norm 0.
              rival [i] = the largest cos(c_i, m_t) over the OTHER speakers t of the same recording with |m_t| > 0, the lowest t at equal
              values, rival_speaker that t (local); none, or |c_i| = 0: rival_speaker = -1 and rival = 0.0.  margin = own - rival.
              mean [s] = m_s / (the windows of speaker s), zeros without windows
  selection   (host; select) a clip is eligible when alone, or when margin >= min_margin (default 0.0: a sample must sound more like the
              rest of its own speaker than like anyone else in the recording - the whole criterion, no tuned number).  Per speaker the
              eligible clips in the order (alone ascending, own descending, solo descending, start ascending); the first max_clips of
              them are taken (None: all), and taking stops before the clip that would carry the total length past
              floor(max_total_s * 16000 + 0.5) samples (None: no cap)

The device path (csrc/samples.hip) serves a pack of recordings on the prefix-sum tables of diarize_ops.GroupTables: sdk_samples_runs, a
segmented scan and a compaction over the packed frame grid that never walks a run (integers only, bit-identical run to run; two waits for
the device per pack: the run counts, then the rows), and sdk_samples_score (float64, fixed summation orders, no floating-point atomics;
the embeddings stay on the device).  runs_host and score_host restate them in numpy.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from pathlib import Path
from typing import TYPE_CHECKING, Dict, List, Optional, Sequence

import numpy as np

from .diarize_host import global_frames
from .segmentation import FRAME_HOP, SAMPLE_RATE
from .words import MAX_WORD_SPEAKERS, gap_frames

if TYPE_CHECKING:
    from .backend import Backend

DEFAULT_MIN_S = 0.5
DEFAULT_MAX_GAP_S = 1.0
FRAME_LEFT = 360                 # frame g covers the samples [270 g + 360, 270 g + 630)
SILENT, OVERLAPPED = -1, -2
ROW_FIELDS = ("speaker", "g0", "g1", "solo")
CLIP_FIELDS = ("speaker", "start", "end", "solo")


@dataclass
class SpeakerSample:
    recording: int               # the index of the recording in the call
    speaker: int                 # local to the recording (the result's numbering)
    start_s: float
    end_s: float
    solo_s: float                # the solo frames the clip carries, in seconds
    own: float
    rival: float
    rival_speaker: int           # -1: none
    alone: bool
    embedding: Optional[np.ndarray] = None     # [d] fp32: the unit mean of the clip's window rows


# ------------------------------------------------------------------------------------------------ the rule on the host
def _seconds_to_samples(who: str, name: str, t: float) -> int:
    t = float(t)
    if not (t == t and 0.0 <= t and t * SAMPLE_RATE + 0.5 < float(1 << 30)):
        raise ValueError(f"{who}: {name}={t} (seconds, >= 0)")
    return int(math.floor(t * SAMPLE_RATE + 0.5))


def min_frames_of(min_s: float) -> int:
    return max(1, -(-_seconds_to_samples("samples", "min_s", min_s) // FRAME_HOP))


def _check_speakers(who: str, K: int):
    if K > MAX_WORD_SPEAKERS:
        raise ValueError(f"{who}: {K} hypothesis speakers; at most {MAX_WORD_SPEAKERS} per recording")


def frame_kinds(speakers, K: int) -> np.ndarray:
    """speakers [G, 2] -> kind [G] int64: SILENT, OVERLAPPED, or k where the frame is solo for k."""
    sp = np.asarray(speakers, dtype=np.int64).reshape(-1, 2)
    K = max(int(K), 0)
    h0, h1 = sp[:, 0], sp[:, 1]
    on0, on1 = (h0 >= 0) & (h0 < K), (h1 >= 0) & (h1 < K)
    return np.where(on0, np.where(on1 & (h1 != h0), OVERLAPPED, h0), np.where(on1, h1, SILENT))


def runs_host(speakers, K: int, gap: int, min_frames: int) -> np.ndarray:
    """sdk_samples_runs for one recording in numpy: speakers [G, 2], its K speakers, gap and min_frames in frames (words.gap_frames,
    min_frames_of) -> rows [N, 4] int32.  As on the device: the frames that are not silent fall into groups that start where the frame
    before them (among those) is missing, of another kind, overlapped or more than gap silent frames away; a solo group is a run."""
    _check_speakers("runs_host", int(K))
    if int(min_frames) < 1 or int(gap) < 0:
        raise ValueError(f"runs_host: gap={gap}, min_frames={min_frames} (gap >= 0, min_frames >= 1)")
    kind = frame_kinds(speakers, K)
    at = np.nonzero(kind != SILENT)[0]
    if at.size == 0:
        return np.zeros((0, 4), np.int32)
    kd = kind[at]
    brk = np.ones(at.size, bool)
    brk[1:] = (kd[1:] != kd[:-1]) | (kd[1:] == OVERLAPPED) | (at[1:] - at[:-1] - 1 > int(gap))
    first = np.nonzero(brk)[0]
    last = np.append(first[1:], at.size) - 1
    solo = last - first + 1                                      # every frame of a solo group is solo
    keep = (kd[first] >= 0) & (solo >= int(min_frames))
    return np.stack([kd[first], at[first], at[last] + 1, solo], 1)[keep].astype(np.int32)


def _cos(dot, na2, nb2):
    with np.errstate(invalid="ignore", divide="ignore"):
        return dot / (np.sqrt(na2) * np.sqrt(nb2))


def score_host(E, clip_off, clip_spk, spk_off):
    """sdk_samples_score in numpy float64: E [W, d] rows, clip_off [M + 1], clip_spk [M] (spk_off[r] + k), spk_off [R + 1] ->
    (mean [S, d] float64, out_f [M, 2] float64 = (own, rival), out_i [M, 3] int32 = (rival_speaker local, windows, alone))."""
    E = np.asarray(E, dtype=np.float64)
    clip_off, clip_spk, spk_off = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (clip_off, clip_spk, spk_off))
    M, S, d = clip_spk.size, int(spk_off[-1]), E.shape[1]
    if clip_off.size != M + 1 or (np.diff(clip_off) < 0).any() or (M and (clip_off[0] < 0 or clip_off[-1] > E.shape[0])):
        raise ValueError(f"score_host: clip_off must hold M + 1 = {M + 1} ascending offsets into the {E.shape[0]} rows")
    if spk_off[0] != 0 or (np.diff(spk_off) < 0).any():
        raise ValueError("score_host: spk_off must hold prefix sums from 0")
    if M and (clip_spk.min() < 0 or clip_spk.max() >= S):
        raise ValueError(f"score_host: clip_spk must lie in [0, {S})")
    c = np.stack([E[a:b].sum(0) for a, b in zip(clip_off[:-1], clip_off[1:])]) if M else np.zeros((0, d))
    m, n_win = np.zeros((S, d)), np.zeros(S, np.int64)
    for i in range(M):                                           # ascending i: the device's order
        m[clip_spk[i]] += c[i]
        n_win[clip_spk[i]] += clip_off[i + 1] - clip_off[i]
    mean = np.where(n_win[:, None] > 0, m / np.maximum(n_win, 1)[:, None], 0.0)
    out_f, out_i = np.zeros((M, 2)), np.zeros((M, 3), np.int32)
    out_i[:, 0], out_i[:, 1] = -1, np.diff(clip_off)
    if M == 0:
        return mean, out_f, out_i
    rest = m[clip_spk] - c
    c2, r2, m2 = (c * c).sum(1), (rest * rest).sum(1), (m * m).sum(1)
    alone = ~(c2 > 0) | ~(r2 > 0)
    out_f[:, 0] = np.where(alone, 0.0, _cos((c * rest).sum(1), c2, r2))
    out_i[:, 2] = alone
    rec = np.searchsorted(spk_off, clip_spk, side="right") - 1
    for i in np.nonzero(c2 > 0)[0]:
        t0, t1 = int(spk_off[rec[i]]), int(spk_off[rec[i] + 1])
        t = np.arange(t0, t1)
        t = t[(t != clip_spk[i]) & (m2[t0:t1] > 0)]
        if t.size:
            cs = _cos(m[t] @ c[i], c2[i], m2[t])
            b = int(np.argmax(cs))                               # the first maximum: the lowest t
            out_f[i, 1], out_i[i, 0] = cs[b], t[b] - t0
    return mean, out_f, out_i


def cut_clips(rows, n_samples: int, max_clip_s: Optional[float] = None, max_candidates: Optional[int] = None) -> np.ndarray:
    """The kept runs of one recording (rows [N, 4]) -> clips [C, 4] int64 = (speaker, start, end, solo), start and end in samples, by
    ascending start: "clips" in the module docstring."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    n_samples = int(n_samples)
    cap = None
    if max_clip_s is not None:
        cap = _seconds_to_samples("cut_clips", "max_clip_s", max_clip_s)
        if cap < 1:
            raise ValueError(f"cut_clips: max_clip_s={max_clip_s} (at least one sample)")
    if max_candidates is not None and int(max_candidates) < 0:
        raise ValueError(f"cut_clips: max_candidates={max_candidates} (None or >= 0)")
    out = []
    for k, g0, g1, solo in rows.tolist():
        s0, s1 = FRAME_HOP * g0 + FRAME_LEFT, min(FRAME_HOP * g1 + FRAME_LEFT, n_samples)
        L = s1 - s0
        if L <= 0:
            raise ValueError(f"cut_clips: the run ({k}, {g0}, {g1}) lies outside the recording's {n_samples} samples")
        n = 1 if cap is None else -(-L // cap)
        for i in range(n):
            out.append((k, s0 + i * L // n, s0 + (i + 1) * L // n, solo // n + (1 if i < solo % n else 0)))
    clips = np.asarray(out, dtype=np.int64).reshape(-1, 4)
    if max_candidates is not None and clips.shape[0]:
        keep = np.zeros(clips.shape[0], bool)
        for k in np.unique(clips[:, 0]):
            idx = np.nonzero(clips[:, 0] == k)[0]
            order = idx[np.lexsort((clips[idx, 1], -clips[idx, 3]))]
            keep[order[:int(max_candidates)]] = True
        clips = clips[keep]
    return clips


def select(clips, own, rival, alone, max_clips: Optional[int] = None, max_total_s: Optional[float] = None, min_margin: float = 0.0) -> Dict[int, List[int]]:
    """clips [C, 4] (cut_clips) of one recording with their scores own, rival [C] and alone [C] -> {speaker: [clip indices]} in the order of
    the rule: "selection" in the module docstring.  A speaker without an eligible clip has no entry."""
    clips = np.asarray(clips, dtype=np.int64).reshape(-1, 4)
    own, rival = np.asarray(own, dtype=np.float64).reshape(-1), np.asarray(rival, dtype=np.float64).reshape(-1)
    alone = np.asarray(alone).reshape(-1).astype(bool)
    C = clips.shape[0]
    if not (own.size == rival.size == alone.size == C):
        raise ValueError(f"select: {own.size} own, {rival.size} rival and {alone.size} alone values for {C} clips")
    if max_clips is not None and int(max_clips) < 0:
        raise ValueError(f"select: max_clips={max_clips} (None or >= 0)")
    min_margin = float(min_margin)
    if min_margin != min_margin:
        raise ValueError("select: min_margin is not a number")
    cap = None if max_total_s is None else _seconds_to_samples("select", "max_total_s", max_total_s)
    ok = alone | (own - rival >= min_margin)
    out: Dict[int, List[int]] = {}
    for k in np.unique(clips[ok, 0]).tolist():
        idx = np.nonzero(ok & (clips[:, 0] == k))[0]
        order = idx[np.lexsort((clips[idx, 1], -clips[idx, 3], -own[idx], alone[idx]))]
        taken, total = [], 0
        for i in order.tolist():
            n = int(clips[i, 2] - clips[i, 1])
            if (max_clips is not None and len(taken) >= int(max_clips)) or (cap is not None and total + n > cap):
                break
            taken.append(i)
            total += n
        if taken:
            out[int(k)] = taken
    return out


# ------------------------------------------------------------------------------------------------ the device path
def _ops():
    import torch
    from . import ops_score
    return torch, ops_score


def runs(eng, results, min_s: float = DEFAULT_MIN_S, max_gap_s: float = DEFAULT_MAX_GAP_S) -> List[np.ndarray]:
    """DiarizationResults (their speakers and n_speakers are read) -> one rows [N_r, 4] int32 per recording: the hypothesis uploaded as
    words.attribute_pack uploads it, sdk_samples_runs, then two downloads (the run counts, then the rows that were written)."""
    from .diarize_ops import GroupTables
    torch, ops_score = _ops()
    results = list(results)
    if not results:
        raise ValueError("samples: no recordings")
    gap, min_frames = gap_frames(max_gap_s), min_frames_of(min_s)
    spk = [np.ascontiguousarray(res.speakers, dtype=np.int32).reshape(-1, 2) for res in results]
    for r, res in enumerate(results):
        _check_speakers(f"samples: recording {r}", int(res.n_speakers))
    R = len(results)
    G_r = [len(sp) for sp in spk]
    n_samples = [FRAME_HOP * g + 226 if g else 0 for g in G_r]                      # a length with global_frames(n) == g: only the grid is read
    tab = GroupTables(eng, np.zeros(R + 1, np.int64), np.concatenate([[0], np.cumsum(G_r)]), n_samples)
    tab.set_clusters(np.concatenate([[0], np.cumsum([max(int(res.n_speakers), 0) for res in results])]))
    speakers_d = torch.from_numpy(np.concatenate(spk)).to(eng.device)
    run_off_d, rows_d = ops_score.samples_runs(eng, speakers_d, tab.frame_off_d, tab.cent_off_d, int(np.diff(tab.cent_off).max()), gap, min_frames)
    run_off = run_off_d.cpu().numpy().astype(np.int64)                               # the first wait
    rows = rows_d[:int(run_off[-1])].cpu().numpy()                                   # the second
    return [rows[int(a):int(b)] for a, b in zip(run_off[:-1], run_off[1:])]


def score(eng, E, clip_off, clip_spk, spk_off):
    """E [W, d] fp32 on the device (it stays there), clip_off [M + 1], clip_spk [M], spk_off [R + 1] host integers -> (mean [S, d] float64,
    out_f [M, 2] float64, out_i [M, 3] int32) on the host: one upload, sdk_samples_score, one download."""
    torch, ops_score = _ops()
    clip_off, clip_spk, spk_off = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (clip_off, clip_spk, spk_off))
    M, R, S = clip_spk.size, spk_off.size - 1, int(spk_off[-1]) if spk_off.size else 0
    if R < 1 or spk_off[0] != 0 or (np.diff(spk_off) < 0).any():
        raise ValueError(f"samples.score: spk_off must hold R + 1 >= 2 prefix sums from 0, got {spk_off.tolist()[:8]}")
    if clip_off.size != M + 1 or (np.diff(clip_off) < 0).any() or clip_off[0] < 0 or clip_off[-1] > int(E.shape[0]):
        raise ValueError(f"samples.score: clip_off must hold M + 1 = {M + 1} ascending offsets into the {int(E.shape[0])} rows of E")
    if M and (clip_spk.min() < 0 or clip_spk.max() >= S):
        raise ValueError(f"samples.score: clip_spk must lie in [0, {S})")
    up = torch.from_numpy(np.concatenate([clip_off, clip_spk, spk_off]).astype(np.int32)).to(eng.device)
    mean, out_f, out_i = ops_score.samples_score(eng, E, up[:M + 1], up[M + 1:2 * M + 1], up[2 * M + 1:], S)
    flat = torch.cat([mean.reshape(-1), out_f.reshape(-1), out_i.reshape(-1).to(torch.float64)]).cpu().numpy()
    d = int(E.shape[1])
    return flat[:S * d].reshape(S, d), flat[S * d:S * d + 2 * M].reshape(M, 2), flat[S * d + 2 * M:].astype(np.int32).reshape(M, 3)


def clip_embeddings(E, bounds) -> np.ndarray:
    """E [W, d] fp32 on the device, bounds [M, 2] (the first row of every clip and the one past its last) -> [M, d] fp32 on the host: the unit
    float64 mean of every clip's rows (Backend.enroll_speaker's arithmetic on a clip), zeros for a clip without rows.  One download."""
    import torch
    bounds = np.asarray(bounds, dtype=np.int64).reshape(-1, 2)
    if bounds.shape[0] == 0:
        return np.zeros((0, int(E.shape[1])), np.float32)
    out = []
    for a, b in bounds.tolist():
        mean = E[a:b].double().mean(dim=0) if b > a else torch.zeros(int(E.shape[1]), dtype=torch.float64, device=E.device)
        out.append((mean / mean.norm().clamp_min(1e-12)).float())
    return torch.stack(out).cpu().numpy()


def as_samples(recording: int, clips, picked: Dict[int, List[int]], out_f, out_i, embeddings=None) -> Dict[int, List[SpeakerSample]]:
    """select's indices -> {speaker: [SpeakerSample]} in the same order; embeddings [C, d] by clip, or None."""
    out: Dict[int, List[SpeakerSample]] = {}
    for k, idx in picked.items():
        out[k] = [SpeakerSample(int(recording), int(k), int(clips[i, 1]) / SAMPLE_RATE, int(clips[i, 2]) / SAMPLE_RATE,
                                int(clips[i, 3]) * FRAME_HOP / SAMPLE_RATE, float(out_f[i, 0]), float(out_f[i, 1]), int(out_i[i, 0]), bool(out_i[i, 2]),
                                None if embeddings is None else np.asarray(embeddings[i], dtype=np.float32)) for i in idx]
    return out


def split_by_recording(tables: Sequence[np.ndarray]) -> np.ndarray:
    """[R] arrays -> the [R + 1] prefix sums of their lengths."""
    return np.concatenate([[0], np.cumsum([len(t) for t in tables])]).astype(np.int64)


# ---- the pipeline on a Backend (backend.py).  Functions of it, not methods: its public surface is pinned name for name; backend.py imports
#      them, so callers reach them as backend.speaker_samples and backend.write_samples.
def speaker_samples(be: Backend, results, samples_or_paths, min_s: float = 0.5, max_gap_s: float = 1.0, max_clip_s=None, max_candidates=None,
                    max_clips=None, max_total_s=None, min_margin: float = 0.0):
    """Which stretches of audio of each diarized speaker are clean enough to listen to and to enrol from: the results of diarize /
    diarize_many and their recordings (16 kHz mono int16 samples, or paths of audio files) -> one {speaker: [samples.SpeakerSample]} per
    recording, a single dict for a single result.  A speaker's runs of solo frames (no overlap, pauses up to max_gap_s bridged, at least
    min_s of solo frames) are found on the device for the whole pack, cut into clips of at most max_clip_s, embedded with the identify
    model (embed_ranges) and scored on the device: own, the cosine of the clip to the rest of its speaker, and rival, its best cosine to
    another speaker of the recording.  A clip is a sample when own - rival >= min_margin (or when it is its speaker's only clip:
    alone); per speaker the best max_clips of them, at most max_total_s in all, best first.  The (start_s, end_s) pairs can be passed
    unchanged as segments= of enroll_speaker; embedding is the unit mean of the clip's windows (samples.py states the rule; parity with
    other toolkits is unpinned)."""
    import torch
    from . import samples as sm
    single = not isinstance(results, (list, tuple))
    results = [results] if single else list(results)
    recs = [samples_or_paths] if single else list(samples_or_paths)
    if len(recs) != len(results):
        raise ValueError(f"speaker_samples: {len(recs)} recordings for {len(results)} results")
    if not results:
        return []
    eng = be.engine()
    recs = [np.asarray(x) for x in be._recordings(recs)]
    for r, (res, pcm) in enumerate(zip(results, recs)):
        if len(res.speakers) != sm.global_frames(len(pcm)):
            raise ValueError(f"speaker_samples: recording {r} has {len(pcm)} samples, its result {len(res.speakers)} frames")
    rows = sm.runs(eng, results, min_s, max_gap_s)
    clips, parts, counts = [], [], []
    for r, pcm in enumerate(recs):
        cl = sm.cut_clips(rows[r], len(pcm), max_clip_s, max_candidates)
        n_win = np.zeros(len(cl), np.int64)
        if len(cl):
            E, _, _, wins, _ = be.embed_ranges(pcm, [(int(a) / sm.SAMPLE_RATE, int(b) / sm.SAMPLE_RATE) for a, b in cl[:, 1:3]])
            if wins:                                                        # in range order: a clip's windows are adjacent rows
                n_win = np.bincount([ri for ri, _, _ in wins], minlength=len(cl)).astype(np.int64)
                parts.append(E)
        clips.append(cl[n_win > 0])                                         # a clip embed_ranges dropped is not a sample
        counts.append(n_win[n_win > 0])
    out = [dict() for _ in results]
    if parts:
        E = torch.cat(parts) if len(parts) > 1 else parts[0]
        clip_off = np.concatenate([[0], np.cumsum(np.concatenate(counts))])
        spk_off = np.concatenate([[0], np.cumsum([max(int(res.n_speakers), 0) for res in results])])
        clip_spk = np.concatenate([spk_off[r] + cl[:, 0] for r, cl in enumerate(clips)])
        _, out_f, out_i = sm.score(eng, E, clip_off, clip_spk, spk_off)
        off = sm.split_by_recording(clips)
        for r, cl in enumerate(clips):
            a, b = int(off[r]), int(off[r + 1])
            picked = sm.select(cl, out_f[a:b, 0], out_f[a:b, 1], out_i[a:b, 2], max_clips, max_total_s, min_margin)
            emb = np.zeros((len(cl), int(E.shape[1])), np.float32)
            chosen = sorted(i for idx in picked.values() for i in idx)
            if chosen:
                emb[chosen] = sm.clip_embeddings(E, np.stack([clip_off[a:b][chosen], clip_off[a + 1:b + 1][chosen]], 1))
            out[r] = sm.as_samples(r, cl, picked, out_f[a:b], out_i[a:b], emb)
    return out[0] if single else out


def write_samples(out_dir, samples, audio) -> List[Path]:
    """One recording's samples ({speaker: [SpeakerSample]}, speaker_samples) and its audio (16 kHz mono int16) ->
    <out_dir>/S<speaker + 1>/sample-NNN.wav (s16le mono 16 kHz) beside sample-NNN.json (the SpeakerSample fields without the embedding),
    NNN from 001 in the order of the list; -> the WAV paths.  The toolkit's .meta.yaml provenance layout is not written."""
    import json
    import wave
    from dataclasses import asdict
    from .samples import SAMPLE_RATE
    audio = np.ascontiguousarray(audio, dtype=np.int16).reshape(-1)
    paths = []
    for k in sorted(samples):
        folder = Path(out_dir) / f"S{int(k) + 1}"
        folder.mkdir(parents=True, exist_ok=True)
        for n, s in enumerate(samples[k], 1):
            a, b = int(round(s.start_s * SAMPLE_RATE)), int(round(s.end_s * SAMPLE_RATE))
            if not 0 <= a < b <= audio.size:
                raise ValueError(f"write_samples: speaker {k} sample {n} ({s.start_s} .. {s.end_s} s) lies outside the recording's {audio.size} samples")
            path = folder / f"sample-{n:03d}.wav"
            with wave.open(str(path), "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(SAMPLE_RATE)
                w.writeframes(audio[a:b].astype("<i2").tobytes())
            meta = {key: val for key, val in asdict(s).items() if key != "embedding"}
            path.with_suffix(".json").write_text(json.dumps(meta, indent=2) + "\n")
            paths.append(path)
    return paths
