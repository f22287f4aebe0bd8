"""Scoring a diarization against a reference annotation: the diarization error rate (DER), computed on the device for a pack of recordings,
and the threshold sweep built on it (diarize.Diarizer.score / sweep, Backend.score_diarization / tune_diarization).  The rule below is THIS
build's statement, following NIST md-eval and pyannote.metrics as published; none of their code is on hand, so PARITY IS UNPINNED and the
tests pin this rule.

  grid        the global frame grid of diarize.py: frame g of a recording has centre sample 270 g + 495, g < global_frames(n_samples).  The
              hypothesis on it is a result's speakers [G, 2] (int32, padded with -1): hypothesis speaker j is active in frame g iff j stands
              in speakers[g]; nhyp(g) = the number of entries >= 0
  reference   per recording a list of (start_s, end_s, name), prepared on the host (prepare_reference): seconds to samples by
              floor(t * 16000 + 0.5) (times must be finite, >= 0 and below 2^31 samples); names numbered 0 .. S - 1 in order of their first
              start (in samples), then by name; per speaker the union of the turns that overlap or abut (sorted by (s0, s1), a turn joins
              the running one when s0 <= its s1), then turns with s1 <= s0 are dropped (a speaker whose turns are all dropped keeps its
              number and is never active).  Reference speaker i is active in frame g iff one of its turns has s0 <= 270 g + 495 < s1;
              nref(g) = the number of active reference speakers
  scored      every frame of the recording, with two exceptions.  collar_s > 0: with c = floor(collar_s * 16000 + 0.5), a frame is not scored
              if some boundary b (an s0 or s1 of a merged reference turn) has |270 g + 495 - b| < c - md-eval's convention, the collar
              applies on each side of the boundary.  skip_overlap=True: a frame with nref >= 2 is not scored.  A UEM (below) removes more.
  UEM         (opt-in: uem=) the un-partitioned evaluation map that DIHARD, AMI and VoxConverse distribute: per recording None (every frame
              is eligible) or a list of (start_s, end_s) (prepare_uem): seconds to samples as above, intervals sorted and merged where they
              overlap or abut (a join when s0 <= the running s1), then intervals with s1 <= s0 dropped.  Frame g is eligible iff one merged
              interval has s0 <= 270 g + 495 < s1; scored becomes the above AND eligible.  The collar still measures from the reference
              boundaries, whatever the UEM.  An empty list scores nothing; an interval may run past the recording's end.  parse_uem reads
              `<uri> <channel> <start> <end>` lines; a uri the file does not hold gets None (uems_for)
  tallies    over the scored frames, all integers: scored (frames), total = sum nref, missed = sum max(0, nref - nhyp), false_alarm =
              sum max(0, nhyp - nref), both = sum min(nref, nhyp), co[i, j] = the frames in which reference i and hypothesis j are both
              active
  mapping     correct = the maximum of sum co[i, m(i)] over maps m that give some reference speakers pairwise different hypothesis speakers
              (an exact maximum-weight assignment); the mapping reported is any map that attains it, pairs with co == 0 reported as
              unmapped (-1); confusion = both - correct.  correct is unique even where the map is not, so every tally is unique
  DER         der = (missed + false_alarm + confusion) / total; with total == 0 it is 0.0 when there is no error, else inf.  Pooled over
              recordings (pool): the ratio of the sums.  Durations are frames * 270 / 16000 s
  JER         (opt-in: jer=True) DIHARD's Jaccard error rate, every reference speaker weighing the same; it follows dscore as published.
              Over the scored frames ref_frames[i] = the frames with reference i active, hyp_frames[j] = the frames that name hypothesis j
              (a name >= K counts for nobody, a name twice in a frame counts once, as in co).  The Jaccard table, int32:
              q[i, j] = floor(co[i, j] * 2^30 / (ref_frames[i] + hyp_frames[j] - co[i, j])) where co[i, j] > 0, else 0, in unsigned 64-bit
              arithmetic (the numerator reaches 2^61, the denominator passes 2^31); its largest value is exactly 2^30.  jsum = the
              maximum-weight assignment on q (the mapping rule above, run on q as it stands), jer_mapping a map that attains it; S' = the
              reference speakers with ref_frames > 0; jer = 1 - jsum / (2^30 S'), and with S' == 0 it is 0.0 when no hyp_frames is positive,
              else 1.0.  Pooled: 1 - sum jsum / (2^30 sum S'), the mean over all reference speakers of all recordings (recordings with
              S' == 0 add nothing to either sum; if sum S' == 0 the pooled value is 0.0 unless one of them had 1.0).  jsum is unique where
              the map is not.  Each q / 2^30 lies within 2^-30 BELOW the true Jaccard index, so jer lies within 2^-30 of the exact rational
              optimum (above it: at most S' pairs, each short by less than 2^-30, divided by S')
  purity      (with jer=True, on the host from the downloaded integers) coverage = sum_i max_j co[i, j] / sum_i ref_frames[i], purity =
              sum_j max_i co[i, j] / sum_j hyp_frames[j]; each is 1.0 when its denominator is 0; pooled: the ratios of the sums
  limits     at most MAX_SCORE_SPEAKERS = 64 reference and 64 hypothesis speakers per recording: more is a ValueError here and refused by
              the library

The device path is three calls in stream order on the prefix-sum tables of diarize_ops.GroupTables (csrc/score.hip): sdk_score_reference
(reference turns -> a 64-bit speaker mask and a scored flag per frame), sdk_score_cooccur (masks and speakers -> co and the tallies, summed per
workgroup in LDS, then integer atomics) and sdk_score_map (one wave per recording: shortest augmenting paths with int64 potentials).  Only
integers, OR and integer adds: the results do not depend on any order and are bit-identical run to run.  The *_host functions restate the three
kernels in numpy; score_host joins them for one recording.  The opt-in parts add calls of csrc/score_jer.hip in the same stream: sdk_score_uem
(a frame's recording and its interval by two binary searches) behind sdk_score_reference, and for jer=True sdk_score_durations (the walk of
sdk_score_cooccur with 64 + 64 counters), sdk_score_jaccard (one thread per cell, an unsigned 64-bit quotient) and sdk_score_map again, on
the Jaccard table.  Integers too, and the same one download.  With uem=None and jer=False no call is added and every result is what it was.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import TYPE_CHECKING, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .diarize_host import global_frames
from .diarize_ops import GroupTables, _check_tensor, _native
from .segmentation import FRAME_FIRST, FRAME_HOP, SAMPLE_RATE   # FRAME_FIRST is re-exported: words.py reads it here

if TYPE_CHECKING:
    from .backend import Backend

MAX_SCORE_SPEAKERS = 64
_INF = 1 << 62
JACCARD_ONE = 1 << 30            # the Jaccard table's unit: q / 2^30 is the index
UEM_EVERYTHING = (0, (1 << 31) - 1)   # the interval a recording without a UEM is handed on the device


@dataclass
class DerResult:
    scored: int                               # frames scored
    total: int                                # reference speaker-frames
    missed: int
    false_alarm: int
    confusion: int
    correct: int
    der: float
    mapping: Dict[object, int]                # reference name -> hypothesis speaker, -1: unmapped ({} for a pooled result)
    co: Optional[np.ndarray]                  # [S, K] int32 co-occurrence (None for a pooled result)
    # With jer=True (None otherwise; the positional constructor above keeps working):
    jer: Optional[float] = None
    jsum: Optional[int] = None                # the Jaccard sum of the best assignment, in units of 2^-30
    ref_speakers: Optional[int] = None        # S': the reference speakers with ref_frames > 0
    ref_frames: Optional[np.ndarray] = None   # [S] int32 (None for a pooled result)
    hyp_frames: Optional[np.ndarray] = None   # [K] int32 (None for a pooled result)
    jer_mapping: Optional[Dict[object, int]] = None   # reference name -> hypothesis speaker under the Jaccard assignment ({} for a pooled result)
    purity: Optional[float] = None
    coverage: Optional[float] = None
    pc_sums: Optional[Tuple[int, int, int, int]] = None   # purity's numerator and denominator, then coverage's: what pool adds up

    @property
    def scored_s(self) -> float:
        return self.scored * FRAME_HOP / SAMPLE_RATE

    @property
    def total_s(self) -> float:
        return self.total * FRAME_HOP / SAMPLE_RATE


@dataclass
class SweepResult:
    thresholds: List[float]
    per_recording: List[List[DerResult]]      # [T][R]
    pooled: List[DerResult]                   # [T]
    best: int                                 # index of the least pooled DER (metric="jer": JER); ties to the threshold nearest PYANNOTE_THRESHOLD, then the lower


@dataclass
class SmoothSweepResult:
    """Diarizer.sweep(smoothing=[pairs]): every threshold under every (min_duration_off, min_duration_on) pair (smooth.py)."""
    thresholds: List[float]
    smoothing: List[Tuple[float, float]]      # [S] the pairs, as given
    per_recording: List[List[List[DerResult]]]    # [T][S][R]
    pooled: List[List[DerResult]]             # [T][S]
    best: Tuple[float, float, float]          # (threshold, min_duration_off, min_duration_on) of the least pooled metric; ties across thresholds as SweepResult.best, then to the earlier pair


def der_value(total: int, missed: int, false_alarm: int, confusion: int) -> float:
    err = int(missed) + int(false_alarm) + int(confusion)
    if total == 0:
        return 0.0 if err == 0 else math.inf
    return err / int(total)


def jer_value(jsum: int, ref_speakers: int, any_hyp: bool = False) -> float:
    """jsum in units of 2^-30 and S' -> 1 - jsum / (2^30 S'); with S' == 0: 1.0 if a hypothesis speaker holds a scored frame, else 0.0."""
    if ref_speakers == 0:
        return 1.0 if any_hyp else 0.0
    return 1.0 - int(jsum) / (JACCARD_ONE * int(ref_speakers))


def pool(results: Sequence[DerResult]) -> DerResult:
    """The summed tallies of many recordings and the ratio of the sums; mapping {} and co None (not comparable across recordings).  Where
    every result carries them, jsum and ref_speakers are summed too (jer: "JER" in the module docstring), and so are purity's and coverage's
    numerators and denominators."""
    s = [sum(int(getattr(r, f)) for r in results) for f in ("scored", "total", "missed", "false_alarm", "confusion", "correct")]
    out = DerResult(*s, der_value(s[1], s[2], s[3], s[4]), {}, None)
    if results and all(r.jsum is not None and r.ref_speakers is not None for r in results):
        out.jsum, out.ref_speakers = sum(int(r.jsum) for r in results), sum(int(r.ref_speakers) for r in results)
        out.jer, out.jer_mapping = jer_value(out.jsum, out.ref_speakers, any(r.ref_speakers == 0 and r.jer == 1.0 for r in results)), {}
    if results and all(r.pc_sums is not None for r in results):
        out.pc_sums = tuple(sum(int(r.pc_sums[k]) for r in results) for k in range(4))
        out.purity, out.coverage = _ratio(*out.pc_sums[:2]), _ratio(*out.pc_sums[2:])
    return out


def best_threshold(thresholds: Sequence[float], pooled: Sequence[DerResult], metric: str = "der") -> int:
    from .cluster import PYANNOTE_THRESHOLD
    return min(range(len(thresholds)), key=lambda t: (getattr(pooled[t], metric), abs(float(thresholds[t]) - PYANNOTE_THRESHOLD), float(thresholds[t])))


def check_metric(who: str, metric: str) -> str:
    if metric not in ("der", "jer"):
        raise ValueError(f"{who}: metric={metric!r} (\"der\" or \"jer\")")
    return metric


# ------------------------------------------------------------------------------------------------ RTTM and the reference on the host
def parse_rttm(text: str) -> Dict[str, List[Tuple[float, float, str]]]:
    """RTTM text -> {uri: [(start_s, end_s, name)]} in file order.  Reads the SPEAKER lines (`SPEAKER <uri> <chan> <start> <dur> <NA> <NA>
    <name> ...`, what diarize_host.to_rttm writes) and ignores every other line."""
    out: Dict[str, List[Tuple[float, float, str]]] = {}
    for n, line in enumerate(text.splitlines(), 1):
        f = line.split()
        if not f or f[0] != "SPEAKER":
            continue
        if len(f) < 8:
            raise ValueError(f"parse_rttm: line {n}: a SPEAKER line has at least 8 fields, got {len(f)}")
        try:
            start, dur = float(f[3]), float(f[4])
        except ValueError:
            raise ValueError(f"parse_rttm: line {n}: start {f[3]!r} and duration {f[4]!r} must be numbers") from None
        out.setdefault(f[1], []).append((start, start + dur, f[7]))
    return out


def references_for(rttm, uris: Sequence[str]) -> List[List[Tuple[float, float, str]]]:
    """An RTTM path or text (or a {uri: turns} dict) and the recordings' uris, in order -> one turn list per recording.  A uri the
    annotation does not hold is a ValueError (an annotation without speech is an empty list in a dict)."""
    if isinstance(rttm, dict):
        table = rttm
    else:
        table = parse_rttm(_text_of(rttm))
    missing = [u for u in uris if u not in table]
    if missing:
        raise ValueError(f"score: the reference holds no uri {missing[:4]} (it has {sorted(table)[:8]})")
    return [list(table[u]) for u in uris]


def to_samples(t: float) -> int:
    if not (t == t and 0.0 <= t and t * SAMPLE_RATE + 0.5 < float(1 << 31)):
        raise ValueError(f"score: time {t} s (finite, >= 0 and below 2^31 samples)")
    return int(math.floor(float(t) * SAMPLE_RATE + 0.5))


def _text_of(source) -> str:
    """A path, or the text itself (anything with a line break, or that names no file)."""
    text = os.fspath(source)
    if "\n" not in text and os.path.exists(text):
        with open(text, "r", encoding="utf-8") as fh:
            text = fh.read()
    return text


def parse_uem(text: str) -> Dict[str, List[Tuple[float, float]]]:
    """UEM text -> {uri: [(start_s, end_s)]} in file order: lines of `<uri> <channel> <start> <end>`; blank lines and lines that start with
    `;` are ignored."""
    out: Dict[str, List[Tuple[float, float]]] = {}
    for n, line in enumerate(text.splitlines(), 1):
        f = line.split()
        if not f or f[0].startswith(";"):
            continue
        if len(f) < 4:
            raise ValueError(f"parse_uem: line {n}: a UEM line has 4 fields (uri, channel, start, end), got {len(f)}")
        try:
            start, end = float(f[2]), float(f[3])
        except ValueError:
            raise ValueError(f"parse_uem: line {n}: start {f[2]!r} and end {f[3]!r} must be numbers") from None
        out.setdefault(f[0], []).append((start, end))
    return out


def uems_for(uem, uris: Sequence[str]) -> List[Optional[List[Tuple[float, float]]]]:
    """A UEM path or text (or a {uri: intervals} dict) and the recordings' uris, in order -> one interval list per recording; a uri the map
    does not hold gets None (scored everywhere), unlike references_for."""
    table = uem if isinstance(uem, dict) else parse_uem(_text_of(uem))
    return [list(table[u]) if u in table else None for u in uris]


def resolve_uems(who: str, uem, uris, n: int):
    """The uem= keyword of the public calls -> None, or one entry (None or an interval list) per recording: a list of n entries, or a UEM
    path / text / {uri: intervals} with the recordings' uris."""
    if uem is None:
        return None
    if isinstance(uem, (str, os.PathLike, dict)):
        if uris is None or len(uris) != n:
            raise ValueError(f"{who}: a UEM file needs uris, one per recording ({n}), got {None if uris is None else len(uris)}")
        return uems_for(uem, list(uris))
    uem = list(uem)
    if len(uem) != n:
        raise ValueError(f"{who}: {len(uem)} UEM entries for {n} recordings")
    return uem


def prepare_uem(uem) -> np.ndarray:
    """None or [(start_s, end_s)] -> the merged intervals [U, 2] int32 (s0, s1) in samples, sorted and disjoint: "UEM" in the module
    docstring.  None gives the one interval UEM_EVERYTHING, an empty list no interval."""
    if uem is None:
        return np.asarray([UEM_EVERYTHING], dtype=np.int32)
    rows = []
    for s0, s1 in sorted((to_samples(a), to_samples(b)) for a, b in uem):
        if rows and s0 <= rows[-1][1]:
            rows[-1][1] = max(rows[-1][1], s1)
        else:
            rows.append([s0, s1])
    return np.asarray([row for row in rows if row[1] > row[0]], dtype=np.int32).reshape(-1, 2)


def uem_mask_host(intervals: np.ndarray, G: int) -> np.ndarray:
    """sdk_score_uem for one recording in numpy: prepare_uem's intervals [U, 2], G frames -> eligible [G] uint8."""
    eligible = np.zeros(G, np.uint8)
    for s0, s1 in np.asarray(intervals, dtype=np.int64).reshape(-1, 2):
        if s1 > s0:
            eligible[int(_first_frame(s0)):min(int(_first_frame(s1)), G)] = 1
    return eligible


def collar_samples(collar_s: float) -> int:
    if not (collar_s == collar_s and 0.0 <= collar_s and collar_s * SAMPLE_RATE + 0.5 < float(1 << 30)):
        raise ValueError(f"score: collar_s={collar_s} (seconds, >= 0)")
    return int(math.floor(float(collar_s) * SAMPLE_RATE + 0.5))


def prepare_reference(turns) -> Tuple[np.ndarray, list]:
    """[(start_s, end_s, name)] -> (merged [M, 3] int32 rows (s0, s1, speaker) by speaker then s0, names [S]): "reference" in the module
    docstring."""
    conv = [(to_samples(a), to_samples(b), name) for a, b, name in turns]
    first: dict = {}
    for s0, _, name in conv:
        first[name] = min(first.get(name, s0), s0)
    names = sorted(first, key=lambda nm: (first[nm], nm))
    rows = []
    for i, name in enumerate(names):
        cur = None
        for s0, s1 in sorted((s0, s1) for s0, s1, nm in conv if nm == name):
            if cur is not None and s0 <= cur[1]:
                cur[1] = max(cur[1], s1)
            else:
                cur = [s0, s1, i]
                rows.append(cur)
    merged = np.asarray([row for row in rows if row[1] > row[0]], dtype=np.int32).reshape(-1, 3)
    return merged, names


def _first_frame(s):
    """The least g >= 0 with 270 g + 495 >= s."""
    a = np.asarray(s, dtype=np.int64) - FRAME_FIRST
    return np.where(a <= 0, 0, (a + FRAME_HOP - 1) // FRAME_HOP)


def reference_masks_host(merged: np.ndarray, G: int, collar: int = 0, skip_overlap: bool = False):
    """sdk_score_reference for one recording in numpy: merged [M, 3], G frames, collar in samples -> (ref_mask [G] uint64, scored [G] uint8)."""
    mask, scored = np.zeros(G, np.uint64), np.ones(G, np.uint8)
    m = np.asarray(merged, dtype=np.int64).reshape(-1, 3)
    for s0, s1, i in m:
        if s1 <= s0 or not 0 <= i < MAX_SCORE_SPEAKERS:
            continue
        mask[int(_first_frame(s0)):min(int(_first_frame(s1)), G)] |= np.uint64(1) << np.uint64(i)
    if skip_overlap:
        scored[_popcount(mask) >= 2] = 0
    if collar > 0:
        for s0, s1, _ in m:
            if s1 > s0:
                for b in (s0, s1):
                    scored[int(_first_frame(b - collar + 1)):min(int(_first_frame(b + collar)), G)] = 0
    return mask, scored


def _popcount(mask: np.ndarray) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(mask, dtype="<u8").view(np.uint8).reshape(-1, 8), axis=1).sum(1).astype(np.int64)


def _active_host(ref_mask: np.ndarray, scored: np.ndarray, speakers: np.ndarray, S: int, K: int):
    """The n scored frames of one recording -> (mask [n] uint64, speakers [n, 2], ref [n, S] bool: reference i is active, hyp [n, K] bool:
    the frame names hypothesis j - named twice counts once)."""
    on = np.asarray(scored).astype(bool)
    mask, sp = np.asarray(ref_mask, dtype=np.uint64)[on], np.asarray(speakers, dtype=np.int64).reshape(-1, 2)[on]
    ref = ((mask[:, None] >> np.arange(S, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    return mask, sp, ref, (sp[:, :, None] == np.arange(K)[None, None, :]).any(1)


def cooccur_host(ref_mask: np.ndarray, scored: np.ndarray, speakers: np.ndarray, S: int, K: int):
    """sdk_score_cooccur for one recording in numpy -> (co [S, K] int32, tally [5] int64: scored, total, missed, false_alarm, both)."""
    mask, sp, ref, hyp = _active_host(ref_mask, scored, speakers, S, K)
    nref, nhyp = _popcount(mask), (sp >= 0).sum(1)
    tally = np.array([len(mask), nref.sum(), np.maximum(nref - nhyp, 0).sum(), np.maximum(nhyp - nref, 0).sum(), np.minimum(nref, nhyp).sum()], np.int64)
    return np.rint(ref.T.astype(np.float64) @ hyp.astype(np.float64)).astype(np.int32).reshape(S, K), tally   # counts below 2^30: exact in float64


def assignment_host(co: np.ndarray):
    """sdk_score_map for one recording in numpy: co [S, K] -> (map [S] int32, correct): the exact maximum-weight assignment on the table
    padded with zeros to square, by shortest augmenting paths on cost = -co with integer potentials (ties to the lower column, as the kernel's
    cross-lane minimum); a pair with co == 0 is reported unmapped."""
    co = np.asarray(co, dtype=np.int64)
    S, K = co.shape
    n = max(S, K)
    w = np.zeros((n, n), np.int64)
    w[:S, :K] = co
    u, v, p = np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, -1, np.int64)
    for i in range(n):
        minv, way, used = np.full(n, _INF, np.int64), np.full(n, -1, np.int64), np.zeros(n, bool)
        j0, i0 = -1, i
        while True:
            cur = -w[i0] - u[i0] - v
            upd = ~used & (cur < minv)
            minv[upd], way[upd] = cur[upd], j0
            cand = np.where(used, _INF, minv)
            j1 = int(np.argmin(cand))
            delta = cand[j1]
            u[p[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            u[i] += delta
            j0 = j1
            used[j0] = True
            i0 = int(p[j0])
            if i0 < 0:
                break
        while j0 >= 0:
            j1 = int(way[j0])
            p[j0] = p[j1] if j1 >= 0 else i
            j0 = j1
    out, correct = np.full(S, -1, np.int32), 0
    for j in range(K):
        if 0 <= p[j] < S and co[p[j], j] > 0:
            out[p[j]] = j
            correct += int(co[p[j], j])
    return out, correct


def durations_host(ref_mask: np.ndarray, scored: np.ndarray, speakers: np.ndarray, S: int, K: int):
    """sdk_score_durations for one recording in numpy -> (ref_frames [S] int32, hyp_frames [K] int32) over the scored frames."""
    _, _, ref, hyp = _active_host(ref_mask, scored, speakers, S, K)
    return ref.sum(0).astype(np.int32).reshape(S), hyp.sum(0).astype(np.int32).reshape(K)


def jaccard_table_host(co: np.ndarray, ref_frames: np.ndarray, hyp_frames: np.ndarray) -> np.ndarray:
    """sdk_score_jaccard for one recording: co [S, K], ref_frames [S], hyp_frames [K] -> q [S, K] int32 in units of 2^-30.  Python integers:
    the numerator passes 2^53.  A denominator of 0 (tables that are no co-occurrence of these durations) gives 0, as on the device."""
    co = np.asarray(co, dtype=np.int64)
    q = np.zeros(co.shape, np.int32)
    for i, j in zip(*np.nonzero(co > 0)):
        den = int(ref_frames[i]) + int(hyp_frames[j]) - int(co[i, j])
        q[i, j] = (int(co[i, j]) << 30) // den if den else 0
    return q


def _ratio(num: int, den: int) -> float:
    return int(num) / int(den) if den else 1.0


def _pc_sums(co, ref_frames, hyp_frames) -> Tuple[int, int, int, int]:
    co = np.asarray(co, dtype=np.int64)
    return (int(co.max(0).sum()) if co.size else 0, int(np.asarray(hyp_frames, dtype=np.int64).sum()),
            int(co.max(1).sum()) if co.size else 0, int(np.asarray(ref_frames, dtype=np.int64).sum()))


def purity_coverage(co: np.ndarray, ref_frames: np.ndarray, hyp_frames: np.ndarray) -> Tuple[float, float]:
    """"purity" in the module docstring -> (purity, coverage)."""
    s = _pc_sums(co, ref_frames, hyp_frames)
    return _ratio(*s[:2]), _ratio(*s[2:])


def _result(names, co, tally, mapping, correct, jer=None) -> DerResult:
    """jer: None, or (ref_frames [S], hyp_frames [K], jsum, jer_mapping [S]) as sdk_score_durations and sdk_score_map on q leave them."""
    scored, total, missed, fa, both = (int(x) for x in tally)
    conf = both - int(correct)
    out = DerResult(scored, total, missed, fa, conf, int(correct), der_value(total, missed, fa, conf),
                    {name: int(mapping[i]) for i, name in enumerate(names)}, np.asarray(co, dtype=np.int32))
    if jer is not None:
        out.ref_frames, out.hyp_frames = np.asarray(jer[0], dtype=np.int32), np.asarray(jer[1], dtype=np.int32)
        out.jsum, out.ref_speakers = int(jer[2]), int((out.ref_frames > 0).sum())
        out.jer = jer_value(out.jsum, out.ref_speakers, bool((out.hyp_frames > 0).any()))
        out.jer_mapping = {name: int(jer[3][i]) for i, name in enumerate(names)}
        out.pc_sums = _pc_sums(out.co, out.ref_frames, out.hyp_frames)
        out.purity, out.coverage = _ratio(*out.pc_sums[:2]), _ratio(*out.pc_sums[2:])
    return out


def _check_counts(who: str, S: int, K: int):
    if S > MAX_SCORE_SPEAKERS or K > MAX_SCORE_SPEAKERS:
        raise ValueError(f"{who}: {S} reference and {K} hypothesis speakers; at most {MAX_SCORE_SPEAKERS} of each per recording")


def score_host(speakers, n_samples: int, reference, collar_s: float = 0.0, skip_overlap: bool = False, uem=None, jer: bool = False) -> DerResult:
    """One recording on the host: speakers [G, 2] int32 (a DiarizationResult's), its n_samples and the reference turns -> DerResult.  The
    numpy restatement of the kernels; K is the largest speaker named, plus one.  uem: None or the recording's [(start_s, end_s)]; jer=True
    fills the result's fields from jer on."""
    sp = np.asarray(speakers, dtype=np.int32).reshape(-1, 2)
    G = global_frames(n_samples)
    if sp.shape[0] != G:
        raise ValueError(f"score_host: speakers holds {sp.shape[0]} frames, {n_samples} samples give {G}")
    merged, names = prepare_reference(reference)
    S, K = len(names), (int(sp.max()) + 1 if sp.size else 0)
    _check_counts("score_host", S, max(K, 0))
    mask, scored = reference_masks_host(merged, G, collar_samples(collar_s), bool(skip_overlap))
    if uem is not None:
        scored &= uem_mask_host(prepare_uem(uem), G)
    co, tally = cooccur_host(mask, scored, sp, S, max(K, 0))
    mapping, correct = assignment_host(co)
    if not jer:
        return _result(names, co, tally, mapping, correct)
    ref_frames, hyp_frames = durations_host(mask, scored, sp, S, max(K, 0))
    jer_mapping, jsum = assignment_host(jaccard_table_host(co, ref_frames, hyp_frames))
    return _result(names, co, tally, mapping, correct, (ref_frames, hyp_frames, jsum, jer_mapping))


# ------------------------------------------------------------------------------------------------ the device path
class PackReference:
    """The references of a pack, prepared (host) and rasterised on the packed frame grid (device): rasterise_references."""
    names: list                  # per recording, the reference names in speaker order
    ref_off: np.ndarray          # [R + 1] int64 prefix sums of the S_r
    max_ref: int
    ref_off_d = None             # [R + 1] int32
    ref_mask = None              # [G] int64 holding the uint64 masks
    scored = None                # [G] uint8


def rasterise_references(eng, tab, references, collar_s: float = 0.0, skip_overlap: bool = False, upload=None, uems=None) -> PackReference:
    """One turn list per recording of the pack (tab: diarize_ops.GroupTables) -> PackReference: sdk_score_reference.  upload: what carries the
    one table of host integers to the device (a caller that counts its transfers passes its own).  uems: None, or per recording None or its
    [(start_s, end_s)]: the merged intervals ride in the same upload and sdk_score_uem runs behind sdk_score_reference."""
    torch, check, _stream = _native()
    if len(references) != tab.R:
        raise ValueError(f"score: {len(references)} references for {tab.R} recordings")
    if uems is not None and len(uems) != tab.R:
        raise ValueError(f"score: {len(uems)} UEM entries for {tab.R} recordings")
    collar = collar_samples(collar_s)
    prepared = [prepare_reference(t) for t in references]
    ref = PackReference()
    ref.names = [names for _, names in prepared]
    for r, names in enumerate(ref.names):
        _check_counts(f"score: recording {r}", len(names), 0)
    ref.ref_off = np.concatenate([[0], np.cumsum([len(n) for n in ref.names])]).astype(np.int64)
    ref.max_ref = max([len(n) for n in ref.names] + [0])
    turn_off = np.concatenate([[0], np.cumsum([len(m) for m, _ in prepared])]).astype(np.int64)
    M, R = int(turn_off[-1]), tab.R
    if M >= (1 << 28):
        raise ValueError(f"score: {M} reference turns in one pack (fewer than 2^28)")
    parts = [turn_off, ref.ref_off] + [m.reshape(-1) for m, _ in prepared]
    if uems is not None:
        merged_uem = [prepare_uem(u) for u in uems]
        uem_off = np.concatenate([[0], np.cumsum([len(m) for m in merged_uem])]).astype(np.int64)
        U = int(uem_off[-1])
        if U >= (1 << 28):
            raise ValueError(f"score: {U} UEM intervals in one pack (fewer than 2^28)")
        parts += [uem_off] + [m.reshape(-1) for m in merged_uem]
    table = np.concatenate(parts).astype(np.int32)
    up = (upload or (lambda a: torch.from_numpy(a).to(eng.device)))(table)                                   # one upload
    turn_off_d, ref.ref_off_d, turns_d = up[:R + 1], up[R + 1:2 * R + 2], up[2 * R + 2:2 * R + 2 + 3 * M]
    ref.ref_mask = torch.empty((max(tab.G, 1),), dtype=torch.int64, device=eng.device)
    ref.scored = torch.empty((max(tab.G, 1),), dtype=torch.uint8, device=eng.device)
    check(eng.lib.sdk_score_reference(eng.ctx, turns_d.data_ptr() if M else None, turn_off_d.data_ptr(), tab.frame_off_d.data_ptr(), ref.ref_off_d.data_ptr(),
                                      R, M, tab.G, ref.max_ref, collar, int(bool(skip_overlap)), ref.ref_mask.data_ptr(), ref.scored.data_ptr(), _stream()),
          "sdk_score_reference")
    if uems is not None:
        a = 2 * R + 2 + 3 * M
        uem_off_d, uem_d = up[a:a + R + 1], up[a + R + 1:]
        check(eng.lib.sdk_score_uem(eng.ctx, uem_d.data_ptr() if U else None, uem_off_d.data_ptr(), tab.frame_off_d.data_ptr(), R, U, tab.G,
                                    ref.scored.data_ptr(), _stream()), "sdk_score_uem")
    ref.ref_mask, ref.scored = ref.ref_mask[:tab.G], ref.scored[:tab.G]
    return ref


@dataclass
class ScoreTables:
    """What score_tables leaves on the device for one pack, by name, and the layout of its one int64 download: pieces() in a fixed order,
    `size` of them, results() to cut a downloaded slice.  The four fields from ref_frames on are None without jer=True."""
    tally: object                             # [R, 5] int64: scored, total, missed, false_alarm, both
    correct: object                           # [R] int64
    mapping: object                           # [sum S_r] int32
    co: object                                # [co_off[-1]] int32: recording r's [S_r, K_r] table at co_off[r]
    co_off: np.ndarray                        # [R + 1] int64, on the host
    cent_off: np.ndarray                      # [R + 1]: the tables' cent_off as it stood at the call
    ref_off: np.ndarray                       # [R + 1]: the reference's
    ref_frames: object = None                 # [sum S_r] int32
    hyp_frames: object = None                 # [sum K_r] int32
    jsum: object = None                       # [R] int64
    jer_mapping: object = None                # [sum S_r] int32

    def _tensors(self) -> list:
        plain = [self.tally, self.correct, self.mapping, self.co]
        return plain if self.jsum is None else plain + [self.ref_frames, self.hyp_frames, self.jsum, self.jer_mapping]

    def pieces(self) -> list:
        """The int64 pieces of the download: tally, correct, map, co, then with jer=True ref_frames, hyp_frames, jsum, jer_mapping."""
        torch = _native()[0]
        return [t.reshape(-1).to(torch.int64) for t in self._tensors()]

    @property
    def size(self) -> int:
        return sum(int(t.numel()) for t in self._tensors())

    def results(self, ref: PackReference, flat: np.ndarray) -> List[DerResult]:
        """The downloaded pieces (numpy, `size` integers) cut into one DerResult per recording."""
        cut = np.cumsum([0] + [int(t.numel()) for t in self._tensors()])
        p = [flat[a:b] for a, b in zip(cut[:-1], cut[1:])]
        tally, out = p[0].reshape(-1, 5), []
        for r, names in enumerate(ref.names):
            a, i0, i1, j0, j1 = (int(v) for v in (self.co_off[r], self.ref_off[r], self.ref_off[r + 1], self.cent_off[r], self.cent_off[r + 1]))
            jer = None if self.jsum is None else (p[4][i0:i1], p[5][j0:j1], p[6][r], p[7][i0:i1])
            out.append(_result(names, np.asarray(p[3][a:a + (i1 - i0) * (j1 - j0)]).reshape(i1 - i0, j1 - j0), tally[r], p[2][i0:i1], p[1][r], jer))
        return out


def score_tables(eng, speakers_dev, tab, ref: PackReference, upload=None, jer: bool = False) -> ScoreTables:
    """speakers [G, 2] int32 on the packed grid (device), tab with clusters set (K_r = the hypothesis speakers of recording r) ->
    ScoreTables, every tensor on the device: sdk_score_cooccur, then sdk_score_map.  Nothing is read back.  jer=True fills ref_frames,
    hyp_frames, jsum and jer_mapping too: sdk_score_durations, sdk_score_jaccard, then sdk_score_map on the Jaccard table."""
    torch, check, _stream = _native()
    if tab.cent_off is None:
        raise ValueError("score: the tables hold no clusters (set_clusters)")
    _check_tensor("score", "speakers", speakers_dev, "int32", (tab.G, 2))
    S_r, K_r = np.diff(ref.ref_off), np.diff(tab.cent_off)
    for r in range(tab.R):
        _check_counts(f"score: recording {r}", int(S_r[r]), int(K_r[r]))
    co_off = np.concatenate([[0], np.cumsum(S_r * K_r)]).astype(np.int64)
    R, total, max_hyp = tab.R, int(co_off[-1]), int(K_r.max()) if K_r.size else 0
    co_off_d = (upload or (lambda a: torch.from_numpy(a).to(eng.device)))(co_off)
    co = torch.empty((max(total, 1),), dtype=torch.int32, device=eng.device)
    tally = torch.empty((R, 5), dtype=torch.int64, device=eng.device)
    mapping = torch.empty((max(int(ref.ref_off[-1]), 1),), dtype=torch.int32, device=eng.device)
    correct = torch.empty((R,), dtype=torch.int64, device=eng.device)
    check(eng.lib.sdk_score_cooccur(eng.ctx, ref.ref_mask.data_ptr() if tab.G else None, ref.scored.data_ptr() if tab.G else None,
                                    speakers_dev.data_ptr() if tab.G else None, tab.frame_off_d.data_ptr(), ref.ref_off_d.data_ptr(), tab.cent_off_d.data_ptr(),
                                    co_off_d.data_ptr(), R, tab.G, ref.max_ref, max_hyp, total, co.data_ptr(), tally.data_ptr(), _stream()), "sdk_score_cooccur")
    check(eng.lib.sdk_score_map(eng.ctx, co.data_ptr(), ref.ref_off_d.data_ptr(), tab.cent_off_d.data_ptr(), co_off_d.data_ptr(), R, ref.max_ref, max_hyp,
                                mapping.data_ptr(), correct.data_ptr(), _stream()), "sdk_score_map")
    n_ref = int(ref.ref_off[-1])
    out = ScoreTables(tally, correct, mapping[:n_ref], co[:total], co_off, tab.cent_off, ref.ref_off)   # set_clusters binds a new cent_off, it never writes into this one
    if not jer:
        return out
    n_hyp = int(tab.cent_off[-1])
    ref_frames = torch.empty((max(n_ref, 1),), dtype=torch.int32, device=eng.device)
    hyp_frames = torch.empty((max(n_hyp, 1),), dtype=torch.int32, device=eng.device)
    q = torch.empty((max(total, 1),), dtype=torch.int32, device=eng.device)
    jer_mapping = torch.empty((max(n_ref, 1),), dtype=torch.int32, device=eng.device)
    jsum = torch.empty((R,), dtype=torch.int64, device=eng.device)
    check(eng.lib.sdk_score_durations(eng.ctx, ref.ref_mask.data_ptr() if tab.G else None, ref.scored.data_ptr() if tab.G else None,
                                      speakers_dev.data_ptr() if tab.G else None, tab.frame_off_d.data_ptr(), ref.ref_off_d.data_ptr(), tab.cent_off_d.data_ptr(),
                                      R, tab.G, ref.max_ref, max_hyp, ref_frames.data_ptr(), hyp_frames.data_ptr(), _stream()), "sdk_score_durations")
    check(eng.lib.sdk_score_jaccard(eng.ctx, co.data_ptr(), ref_frames.data_ptr(), hyp_frames.data_ptr(), ref.ref_off_d.data_ptr(), tab.cent_off_d.data_ptr(),
                                    co_off_d.data_ptr(), R, total, q.data_ptr(), _stream()), "sdk_score_jaccard")
    check(eng.lib.sdk_score_map(eng.ctx, q.data_ptr(), ref.ref_off_d.data_ptr(), tab.cent_off_d.data_ptr(), co_off_d.data_ptr(), R, ref.max_ref, max_hyp,
                                jer_mapping.data_ptr(), jsum.data_ptr(), _stream()), "sdk_score_map")
    out.ref_frames, out.hyp_frames, out.jsum, out.jer_mapping = ref_frames[:n_ref], hyp_frames[:n_hyp], jsum, jer_mapping[:n_ref]
    return out


def score_grouped(eng, speakers_dev, tab, references, collar_s: float = 0.0, skip_overlap: bool = False, uems=None, jer: bool = False) -> List[DerResult]:
    """The device path for one pack: speakers [G, 2] int32 on the packed frame grid of tab (diarize_ops.GroupTables with clusters set), one
    reference turn list per recording -> one DerResult per recording.  Three kernels calls, then one download of the integer tables.  uems:
    None, or one entry per recording (None or its UEM intervals): one more call; jer=True: three more, the same one download."""
    ref = rasterise_references(eng, tab, references, collar_s, skip_overlap, uems=uems)
    tables = score_tables(eng, speakers_dev, tab, ref, jer=jer)
    return tables.results(ref, _native()[0].cat(tables.pieces()).cpu().numpy())


def score_results(eng, results, references, collar_s: float = 0.0, skip_overlap: bool = False, uems=None, jer: bool = False) -> List[DerResult]:
    """Diarizer.score: DiarizationResults and one reference turn list per result -> one DerResult per result; their `speakers` are uploaded
    and scored on the device as one pack (score_grouped)."""
    results, references = list(results), list(references)
    if len(references) != len(results):
        raise ValueError(f"score: {len(references)} references for {len(results)} recordings")
    if uems is not None and len(uems) != len(results):
        raise ValueError(f"score: {len(uems)} UEM entries for {len(results)} recordings")
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
    tab = GroupTables(eng, np.zeros(len(results) + 1, np.int64), np.concatenate([[0], np.cumsum(G_r)]), n_samples)
    tab.set_clusters(np.concatenate([[0], np.cumsum([int(res.n_speakers) for res in results])]))
    return score_grouped(eng, torch.from_numpy(np.concatenate(spk)).to(eng.device), tab, references, collar_s, skip_overlap, uems, jer)


# ---- scoring the DIHARD way.  A function of a Backend (backend.py), not a method of it: Backend.score_diarization keeps its signature;
#      backend.py imports it, so callers reach it as backend.score_diarization_uem.
def score_diarization_uem(be: Backend, results, references, uris=None, collar_s: float = 0.0, skip_overlap: bool = False, uem=None, jer: bool = False):
    """Backend.score_diarization with an evaluation map and the Jaccard error rate.  uem: the map outside which nothing is scored - one
    entry per result (None, or a list of (start_s, end_s)), or the path or text of a UEM file (or {uri: intervals}) read with `uris`; a
    uri it does not hold is scored everywhere.  jer=True: every score.DerResult carries the Jaccard error rate (jer, jsum, ref_speakers,
    ref_frames, hyp_frames, jer_mapping), purity and coverage beside the DER; score.pool(list) pools them too.  With uem=None and
    jer=False it is score_diarization.  Backend.tune_diarization takes the same two keywords, and metric="jer"."""
    results = list(results)
    return be.diarizer().score(results, be._references("score_diarization_uem", references, uris, len(results)), collar_s, skip_overlap,
                               uem=uem, jer=jer, uris=uris)
