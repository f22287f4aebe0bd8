"""Smoothing of the diarized turns: a speaker's short pauses are filled and the short turns are dropped, on the device, before the per-frame
speakers of a diarization (diarize.DiarizationResult.speakers) are cut into turns (Diarizer.run / run_many / sweep: min_duration_off,
min_duration_on, smoothing=; backend.smooth_diarization for finished results).  The rule below is THIS build's statement; it follows the
order of PyAnnote's Binarize as published, fill then drop, but none of its code is on hand, so PARITY IS UNPINNED and the tests pin this rule.

  grid        that of score.py / samples.py: frame g of a recording has centre sample 270 g + 495, g < G = global_frames(n_samples).  The
              hypothesis is speakers [G, 2] (int32) on the packed frame grid of a pack, with frame_off [R + 1], K_r = the speakers of
              recording r (cent_off) and cap = diarize_host._speaker_cap(max_speakers), 1 or 2
  kinds       an entry < 0 or >= K_r names nobody; a speaker named twice in a frame counts once.  a_k[g] = frame g names k
  frames      fill = floor(min_duration_off * 16000 + 0.5) // 270 (words.gap_frames: a pause is filled when it is no longer than the time);
              keep = ceil(floor(min_duration_on * 16000 + 0.5) / 270), 0 for 0 (a turn stays when it is no shorter than the time).  The
              times are checked like samples._seconds_to_samples, and both counts are at most MAX_SMOOTH_FRAMES = 1024 (about 17 s): more
              is a ValueError here and refused by the library
  1 fill      a gap of k is a maximal stretch [g0, g1) with a_k = 0 whose frames g0 - 1 and g1 both lie inside the same recording and both
              name k: a stretch at the start or the end of a recording is no gap and nothing reaches across a recording boundary.  k is a
              FILLER of frame g when g lies in a gap of k with g1 - g0 <= fill.  The fillers are decided on the input table alone
  2 cap       frame g of the INTERMEDIATE table names first the speakers the input frame names, in slot order, each once, compacted to the
              low slots, then its fillers in ascending k until cap speakers stand; the rest is -1.  A filler never displaces a speaker
              the stitching put there (cap = 1 and two speakers named: both stay), and with max_speakers=1 an exclusive diarization stays
              exclusive
  3 drop      in the intermediate table a run of k is a maximal stretch of consecutive frames of one recording that name k.  With keep > 0
              every run shorter than keep frames is removed; what remains of a frame is compacted to the low slots in the same order.  A
              filled gap that lost a frame to the cap leaves two runs, judged separately
  tallies     per recording two int32: filled = the (frame, speaker) pairs named by the intermediate table and not by the input, dropped =
              the pairs named by the intermediate table and not by the output
  unchanged   count stays the segmentation's estimate; n_speakers, the numbering, labels, centroids and scores stay as they are: a
              speaker who loses every frame keeps their number and has no turn
  canonical   with fill = keep = 0 the kernels return the table with every entry that names nobody set to -1, duplicates removed and the
              slots compacted.  The public keywords at 0 do not enter the path at all: every result is what it was

The device path (csrc/smooth.hip, sdk_smooth_turns) serves a pack on the prefix-sum tables of diarize_ops.GroupTables in three launches of
one thread per frame, SMOOTH_BLOCK_FRAMES = 256 frames a workgroup, without per-speaker memory (the cost does not depend on K_r): per entry
the distance to the next frame that names the same speaker, looked for over fill + 1 frames; per frame the fill frames to its left, where an
entry whose distance reaches past the frame is the one run end whose gap covers it; per entry of the intermediate table the run around it,
counted over at most keep - 1 frames to each side.  Integers only, integer atomic sums for the tallies: bit-identical run to run.  Nothing
waits for the device.  smooth_host restates it in numpy, speaker by speaker.
"""
from __future__ import annotations

from typing import TYPE_CHECKING, List, Optional, Sequence, Tuple

import numpy as np

from .samples import _seconds_to_samples
from .segmentation import FRAME_HOP
from .words import gap_frames

if TYPE_CHECKING:
    from .backend import Backend

MAX_SMOOTH_FRAMES = 1024         # the longest fill and keep, in frames (SMT_MAX_FRAMES of csrc/smooth.hip): 1024 * 270 / 16000 = 17.28 s
SMOOTH_BLOCK_FRAMES = 256        # the packed frames one workgroup of sdk_smooth_turns serves (SMT_NT); the walks read across its edges from memory


# ------------------------------------------------------------------------------------------------ the rule on the host
def fill_frames_of(min_duration_off: float) -> int:
    """Seconds -> fill, in frames ("frames" in the module docstring)."""
    _seconds_to_samples("smooth", "min_duration_off", min_duration_off)
    fill = gap_frames(float(min_duration_off))
    if fill > MAX_SMOOTH_FRAMES:
        raise ValueError(f"smooth: min_duration_off={min_duration_off} is {fill} frames; at most {MAX_SMOOTH_FRAMES}")
    return fill


def keep_frames_of(min_duration_on: float) -> int:
    """Seconds -> keep, in frames ("frames" in the module docstring)."""
    keep = -(-_seconds_to_samples("smooth", "min_duration_on", min_duration_on) // FRAME_HOP)
    if keep > MAX_SMOOTH_FRAMES:
        raise ValueError(f"smooth: min_duration_on={min_duration_on} is {keep} frames; at most {MAX_SMOOTH_FRAMES}")
    return keep


def _check_frames(who: str, fill, keep, cap) -> Tuple[int, int, int]:
    fill, keep, cap = int(fill), int(keep), int(cap)
    if not (0 <= fill <= MAX_SMOOTH_FRAMES and 0 <= keep <= MAX_SMOOTH_FRAMES):
        raise ValueError(f"{who}: fill={fill}, keep={keep} (frames, 0 .. {MAX_SMOOTH_FRAMES})")
    if cap not in (1, 2):
        raise ValueError(f"{who}: cap={cap} (1 or 2 speakers per frame)")
    return fill, keep, cap


def _offsets(who: str, frame_off, cent_off, G: int):
    frame_off, cent_off = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (frame_off, cent_off))
    R = frame_off.size - 1
    if R < 1 or frame_off[0] != 0 or (np.diff(frame_off) < 0).any() or frame_off[-1] != G:
        raise ValueError(f"{who}: frame_off must hold R + 1 >= 2 prefix sums from 0 to the {G} frames, got {frame_off.tolist()[:8]}")
    if cent_off.shape != (R + 1,) or (np.diff(cent_off) < 0).any():
        raise ValueError(f"{who}: cent_off must hold R + 1 = {R + 1} prefix sums, got {cent_off.tolist()[:8]}")
    return frame_off, cent_off, R


def _runs(a: np.ndarray):
    """a [n] bool -> (first [m], last + 1 [m]) of its maximal runs of True."""
    edge = np.diff(np.concatenate([[0], a.astype(np.int8), [0]]))
    return np.nonzero(edge == 1)[0], np.nonzero(edge == -1)[0]


def canonical(speakers, K: int) -> np.ndarray:
    """One recording's speakers [G, 2] -> the canonical form [G, 2] int32 ("canonical" in the module docstring)."""
    sp = np.asarray(speakers, dtype=np.int64).reshape(-1, 2)
    h0, h1 = sp[:, 0], sp[:, 1]
    on0 = (h0 >= 0) & (h0 < max(int(K), 0))
    on1 = (h1 >= 0) & (h1 < max(int(K), 0)) & ~(on0 & (h1 == h0))
    return np.stack([np.where(on0, h0, np.where(on1, h1, -1)), np.where(on0 & on1, h1, -1)], 1).astype(np.int32)


def _smooth_recording(speakers, K: int, fill: int, keep: int, cap: int):
    """The rule for one recording -> (speakers [G, 2] int32, filled, dropped)."""
    mid = canonical(speakers, K)
    named = np.unique(mid[mid >= 0]).tolist()
    n = (mid >= 0).sum(1)
    filled = 0
    for k in named if fill > 0 else []:                              # ascending k: the order in which the fillers take the free slots
        a = (mid[:, :2] == k).any(1)                                 # read before anything of k is written: k's own entries are the input's
        first, end = _runs(a)
        want = np.zeros(len(a), bool)
        for g0, g1 in zip(end[:-1].tolist(), first[1:].tolist()):    # the stretch between two runs of k
            if g1 - g0 <= fill:
                want[g0:g1] = True
        at = np.nonzero(want & (n < cap))[0]
        mid[at, n[at]] = k
        n[at] += 1
        filled += len(at)
    out = mid.copy()
    dropped = 0
    for k in named if keep > 1 else []:
        a = (mid == k).any(1)
        for g0, g1 in zip(*(v.tolist() for v in _runs(a))):
            if g1 - g0 < keep:
                out[g0:g1][mid[g0:g1] == k] = -1
                dropped += g1 - g0
    hole = (out[:, 0] < 0) & (out[:, 1] >= 0)
    out[hole, 0], out[hole, 1] = out[hole, 1], -1
    return out, filled, dropped


def smooth_host(speakers, frame_off, cent_off, fill: int, keep: int, cap: int):
    """sdk_smooth_turns in numpy: speakers [G, 2] on the packed frame grid, frame_off and cent_off [R + 1], fill and keep in frames
    (fill_frames_of, keep_frames_of), cap 1 or 2 -> (speakers [G, 2] int32, tallies [R, 2] int32 = (filled, dropped))."""
    fill, keep, cap = _check_frames("smooth_host", fill, keep, cap)
    sp = np.asarray(speakers, dtype=np.int32).reshape(-1, 2)
    frame_off, cent_off, R = _offsets("smooth_host", frame_off, cent_off, sp.shape[0])
    out, tallies = np.full(sp.shape, -1, np.int32), np.zeros((R, 2), np.int32)
    for r in range(R):
        a, b = int(frame_off[r]), int(frame_off[r + 1])
        out[a:b], tallies[r, 0], tallies[r, 1] = _smooth_recording(sp[a:b], int(cent_off[r + 1] - cent_off[r]), fill, keep, cap)
    return out, tallies


def smoothing_fields(min_duration_off: float, min_duration_on: float, fill: int, keep: int, tally) -> dict:
    """DiarizationResult.smoothing of one recording."""
    return {"min_duration_off": float(min_duration_off), "min_duration_on": float(min_duration_on), "fill": int(fill), "keep": int(keep),
            "filled": int(tally[0]), "dropped": int(tally[1])}


def check_pairs(who: str, smoothing) -> Optional[List[Tuple[float, float, int, int]]]:
    """The smoothing= keyword of sweep: None, or a list of (min_duration_off, min_duration_on) -> [(off, on, fill, keep)]."""
    if smoothing is None:
        return None
    pairs = [tuple(p) for p in smoothing]
    if not pairs or any(len(p) != 2 for p in pairs):
        raise ValueError(f"{who}: smoothing={smoothing!r} (None, or a list of at least one (min_duration_off, min_duration_on) pair)")
    return [(float(a), float(b), fill_frames_of(a), keep_frames_of(b)) for a, b in pairs]


# ------------------------------------------------------------------------------------------------ the device path
def smooth_turns(eng, speakers_dev, tab_or_offsets, fill: int, keep: int, cap: int):
    """speakers [G, 2] int32 on the packed frame grid (device; NOT changed), the pack's tables - a diarize_ops.GroupTables with clusters
    set, or the pair (frame_off, cent_off) of [R + 1] int32 device tensors - and fill, keep in frames, cap 1 or 2 -> (smoothed speakers
    [G, 2] int32, tallies [R, 2] int32) on the device: sdk_smooth_turns on a copy.  Nothing waits."""
    import torch
    from . import _args
    from ._lib import check
    from .ops import _stream
    who = "smooth_turns"
    fill, keep, cap = _check_frames(who, fill, keep, cap)
    G = int(_args.tensor(who, "speakers", speakers_dev, "int32", (None, 2)).shape[0])
    if isinstance(tab_or_offsets, (tuple, list)):
        frame_off, cent_off = tab_or_offsets
    else:
        if tab_or_offsets.cent_off_d is None:
            raise ValueError("smooth_turns: the tables hold no clusters (set_clusters)")
        frame_off, cent_off = tab_or_offsets.frame_off_d, tab_or_offsets.cent_off_d
        if tab_or_offsets.G != G:
            raise ValueError(f"smooth_turns: speakers holds {G} frames, the tables {tab_or_offsets.G}")
    R = int(_args.tensor(who, "frame_off", frame_off, "int32", (None,)).shape[0]) - 1
    if R < 1:
        raise ValueError(f"smooth_turns: frame_off must hold R + 1 >= 2 prefix sums, got {list(frame_off.shape)}")
    _args.tensor(who, "cent_off", cent_off, "int32", (R + 1,))
    if G >= 1 << 30:
        raise ValueError(f"smooth_turns: G={G} frames in one pack (fewer than 2^30)")
    out = speakers_dev.clone()
    tallies = torch.empty((R, 2), dtype=torch.int32, device=speakers_dev.device)
    ws = eng._workspace("sdk_smooth_turns_workspace_bytes", G)
    check(eng.lib.sdk_smooth_turns(eng.ctx, out.data_ptr() if G else None, frame_off.data_ptr(), cent_off.data_ptr(), R, G, fill, keep, cap,
                                   tallies.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "sdk_smooth_turns")
    return out, tallies


def smooth_results(eng, results: Sequence, min_duration_off: float = 0.0, min_duration_on: float = 0.0, max_speakers: Optional[int] = None) -> list:
    """backend.smooth_diarization: finished DiarizationResults -> copies with speakers, turns and smoothing replaced.  Their speakers tables go
    up as one pack (one upload), through sdk_smooth_turns once, and come down with the tallies in one download."""
    import copy

    import torch
    from .diarize_host import _speaker_cap, turns_from_frames
    results = list(results)
    fill, keep = fill_frames_of(min_duration_off), keep_frames_of(min_duration_on)
    if max_speakers is not None and int(max_speakers) < 0:
        raise ValueError(f"max_speakers={max_speakers}: must be None or >= 0")
    if not results:
        return []
    spk = [np.ascontiguousarray(res.speakers, dtype=np.int32).reshape(-1, 2) for res in results]
    R, G_r, K_r = len(results), [len(sp) for sp in spk], [max(int(res.n_speakers), 0) for res in results]
    frame_off, cent_off = np.concatenate([[0], np.cumsum(G_r)]), np.concatenate([[0], np.cumsum(K_r)])
    G = int(frame_off[-1])
    if G >= 1 << 30:
        raise ValueError(f"smooth: {G} frames in one call (fewer than 2^30)")
    up = torch.from_numpy(np.concatenate([frame_off, cent_off] + [sp.reshape(-1) for sp in spk]).astype(np.int32)).to(eng.device)      # one upload
    sp_d, tallies = smooth_turns(eng, up[2 * R + 2:].reshape(G, 2), (up[:R + 1], up[R + 1:2 * R + 2]), fill, keep, max(_speaker_cap(max_speakers), 1))
    flat = torch.cat([sp_d.reshape(-1), tallies.reshape(-1)]).cpu().numpy()                                                            # one download
    sp_h, tl = flat[:2 * G].reshape(G, 2), flat[2 * G:].reshape(R, 2)
    out = []
    for r, res in enumerate(results):
        new = copy.copy(res)
        new.speakers = sp_h[int(frame_off[r]):int(frame_off[r + 1])].copy()
        new.turns = turns_from_frames(new.speakers, K_r[r])
        new.smoothing = smoothing_fields(min_duration_off, min_duration_on, fill, keep, tl[r])
        out.append(new)
    return out


# ---- smoothing finished results.  A function of a Backend (backend.py), not a method of it (its public surface is pinned name for name);
#      backend.py imports it, so callers reach it as backend.smooth_diarization.
def smooth_diarization(be: Backend, results, min_duration_off: float = 0.0, min_duration_on: float = 0.0, max_speakers=None):
    """The results of diarize / diarize_many / a closed stream with their turns smoothed: a speaker's pauses no longer than
    min_duration_off seconds are filled (where the frame has a free slot: at most 2 speakers per frame, fewer with max_speakers, and a
    speaker the diarization put there is never displaced), then the turns shorter than min_duration_on seconds are dropped - PyAnnote's
    Binarize hyper-parameters, in its order.  -> copies of the results with speakers, turns and smoothing ({min_duration_off,
    min_duration_on, fill, keep, filled, dropped}) replaced; everything else, count included, is what it was.  One upload, one launch
    sequence (sdk_smooth_turns) and one download for the whole list; a single result gives a single result.  diarize(min_duration_off=,
    min_duration_on=) does the same before the table comes down (smooth.py states the rule; parity with PyAnnote is unpinned)."""
    from .smooth import smooth_results
    single = not isinstance(results, (list, tuple))
    out = smooth_results(be.engine(), [results] if single else list(results), min_duration_off, min_duration_on, max_speakers)
    return out[0] if single else out
