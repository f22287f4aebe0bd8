"""Streaming speaker diarization - "who is speaking now", a bounded delay after the audio arrives: the chunks of diarize.py embedded as they
become due, a speaker inventory that grows online, and a rolling stitch that emits frames once their latency has passed.  The rule follows the
published description of online diarization with local segmentation and incremental constrained clustering (Coria et al. 2021, the "diart"
design) as best known here; no code of it is on hand, so PARITY IS UNPINNED, as with the batch pipeline, and the tests pin THIS rule.

  parameters  step_s (0.5; hop = round(step_s * 16000) >= 270 samples), latency_s (step_s; step_s <= latency_s <= 10), capacity (20; the size
              of a stream's speaker table, 1 .. 64), delta_new (1.0; a cosine distance, 0 .. 2), max_speakers (the cap PER FRAME of diarize.py)
  chunks      the chunks of a stream of n samples are exactly segmentation.chunk_starts(n, step_s): chunk j (start j * hop) is due as soon as
              j * hop + CHUNK samples have arrived; finish() adds the chunk that ends at the stream's end when (n - CHUNK) % hop != 0, and the
              single zero-padded chunk at 0 when n <= CHUNK.  A stream with no samples is empty.
  embedding   Diarizer.embed_chunks, unchanged: cls [F], info [3, 4] and three unit rows per chunk.  The candidates of a chunk are its
              diarize_host.candidate_mask rows; a candidate is LONG when it is in diarize_host.training_mask (TRAIN_CLEAN_DEN * clean_frames >= F).
              Rows that are no candidates are never read.
  inventory   K <= capacity speakers; per speaker the float64 sum S_k of the unit fp32 rows added to it and their number n_k; its unit
              centroid is S_k / ||S_k||.  Speakers are numbered in the order in which they are founded and never renumbered.  A cosine is the
              float64 dot product of a row with a unit centroid.
  mapping     of a chunk with m candidates.
              K = 0: every long candidate, in slot order, founds a speaker while K < capacity; every other candidate gets -1.
              K > 0: first the constrained assignment of diarize.py on the K unit centroids (the same rule, tie order and n = min(m, K)).
              Then, in slot order: candidate i with label k is MATCHED when k >= 0 and 1 - cos(i, k) <= delta_new.  A matched long candidate
              adds its row to S_k and n_k grows by one (a centroid takes at most one row per step, so the order is fixed).  An unmatched long
              candidate founds a speaker while K < capacity and its label becomes the new id.  Every other candidate keeps its constrained
              label, -1 included, and changes nothing.  A speaker founded in a step is not offered to the other candidates of that step.
  score       the cosine to the centroid as it stood BEFORE the update; 1 for a founder, 0 where the label is -1
  stitching   on diarize.py's global frame grid (frame g, centre 270 g + 495, is frame g + q_c of chunk c, q_c = (135 - start_c) // 270).
              act[g, k], the chunk count nc[g] and the count sum live in a ring of RING = 1024 frames per stream.
              hold = (round(latency_s * 16000) - hop) // 270 frames.  After chunk c the stream emits every frame not yet emitted with
              g < F - q_c - hold (a chunk that finish() adds: and g < global_frames(n) - the zero-padded chunk reaches beyond the
              stream's end); finish() then emits the rest, up to global_frames(n).  An emitted frame's count and speakers follow
              diarize_host.reconstruct_host's rule on the chunks that have contributed SO FAR (the mean count rounded half up and capped; the
              clusters of largest act > 0, ties to the lower id).  Emitted frames never change: a later chunk's verdict on them is dropped.
              With latency_s = 10 and (n - CHUNK) % hop == 0 every frame is emitted after its last chunk, so the stream's frames are
              reconstruct_host's on its own labels; a shorter latency trades chunks per frame for delay, and the final off-grid chunk of
              finish() may find frames it overlaps already emitted.
  bank        StreamBank steps R streams together: while any stream has a chunk due, ONE batched embed_chunks over the due chunks of all
              streams, then ONE sdk_stream_step launch (csrc/stream.hip: one workgroup per stream; tables, sums and rings stay in one device
              block that the host never reads to take a step), then ONE download: the step's labels and emitted frames.  Each stream's audio
              crosses to the device once, into its slot of a bank buffer from which the due chunks are cut by a start table.

The *_host functions restate sdk_stream_step and sdk_stream_flush in numpy (HostStream holds what the device block holds, ring included);
tests/stream_ref.py restates the rule a second time without the ring.  Re-clustering or merging of online speakers is out of scope: a
speaker founded twice stays two (diarize_link.link_speakers joins inventories after the fact).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

from .diarize_host import (N_LOCAL, DiarizationResult, _COUNT, _MASK, _speaker_cap, candidate_mask, constrained_chunk,
                           global_frames, training_mask, turns_from_frames)
from .segmentation import CHUNK, FRAME_HOP, SAMPLE_RATE
from .segmentation import num_frames as seg_frames

RING = 1024                      # frames a stream's ring holds (SDK_STREAM_RING)
MAX_CAPACITY = 64                # SDK_STREAM_MAX_SPEAKERS
MAX_LATENCY_S = 10.0             # a chunk: no frame waits longer for its last chunk
SLOT = 2 * CHUNK                 # samples of a stream's slot in the bank buffer: the last chunk's worth kept, a chunk's worth of room


# ------------------------------------------------------------------------------------------------ parameters and the chunk schedule
def check_stream_options(step_s: float = 0.5, latency_s: Optional[float] = None, capacity: int = 20, delta_new: float = 1.0,
                         max_speakers: Optional[int] = None) -> Tuple[int, int, int]:
    """The constructor's refusals -> (hop, latency in samples, hold in frames)."""
    if not (isinstance(step_s, (int, float)) and np.isfinite(step_s) and step_s > 0):
        raise ValueError(f"stream: step_s={step_s!r} (seconds, positive)")
    hop = int(round(step_s * SAMPLE_RATE))
    if hop < FRAME_HOP:
        raise ValueError(f"stream: step_s={step_s} is hop={hop} samples (at least {FRAME_HOP}, one frame)")
    latency_s = step_s if latency_s is None else latency_s
    if not (isinstance(latency_s, (int, float)) and step_s <= latency_s <= MAX_LATENCY_S):
        raise ValueError(f"stream: latency_s={latency_s!r} (step_s={step_s} .. {MAX_LATENCY_S})")
    if not (isinstance(capacity, (int, np.integer)) and 1 <= capacity <= MAX_CAPACITY):
        raise ValueError(f"stream: capacity={capacity!r} (1 .. {MAX_CAPACITY} speakers per stream)")
    if not (isinstance(delta_new, (int, float)) and np.isfinite(delta_new) and 0.0 <= delta_new <= 2.0):
        raise ValueError(f"stream: delta_new={delta_new!r} (a cosine distance, finite, 0 .. 2)")
    if max_speakers is not None and int(max_speakers) < 0:
        raise ValueError(f"max_speakers={max_speakers}: must be None or >= 0")
    latency = max(hop, int(round(latency_s * SAMPLE_RATE)))
    return hop, latency, (latency - hop) // FRAME_HOP


class ChunkSchedule:
    """Which chunks of a stream are due ("chunks" in the module docstring): host integers only."""

    def __init__(self, hop: int):
        self.hop, self.n, self.done, self.finished = int(hop), 0, 0, False      # samples arrived, chunks handed out

    def due(self, n_new: int = 0) -> int:
        """How many grid chunks would be due with n_new more samples."""
        n = self.n + int(n_new)
        return 0 if n < CHUNK else max(0, (n - CHUNK) // self.hop + 1 - self.done)

    def push(self, n_new: int) -> List[int]:
        """n_new more samples -> the starts of the chunks that become due, in order."""
        if self.finished:
            raise ValueError("stream: push to a finished stream (reset it first)")
        k = self.due(n_new)
        self.n += int(n_new)
        out = [(self.done + i) * self.hop for i in range(k)]
        self.done += k
        return out

    def finish(self) -> Optional[int]:
        """The end of the stream -> the start of its last chunk, or None when the grid chunks reach the end (or the stream is empty)."""
        if self.finished:
            raise ValueError("stream: finished already (reset it first)")
        assert self.due(0) == 0, "every due chunk is handed out before the end"
        self.finished = True
        if self.n == 0:
            return None
        if self.n <= CHUNK:
            return None if self.done else 0                      # n == CHUNK: the chunk at 0 was a grid chunk
        return None if (self.n - CHUNK) % self.hop == 0 else self.n - CHUNK


def chunk_q(start: int) -> int:
    return (135 - int(start)) // FRAME_HOP


# ------------------------------------------------------------------------------------------------ host restatement (numpy)
class HostStream:
    """What the device block holds for one stream: K, sums, counts, the emission frontier, the ring and its reach."""

    def __init__(self, capacity: int, d: int):
        self.capacity, self.d, self.K = int(capacity), int(d), 0
        self.S, self.n = np.zeros((capacity, d)), np.zeros(capacity, np.int64)
        self.frontier = self.reach = 0
        self.nc, self.cnt, self.act = np.zeros(RING, np.int64), np.zeros(RING, np.int64), np.zeros((RING, capacity), np.int64)

    def centroids(self) -> np.ndarray:
        """[K, d] float64 unit rows."""
        S = self.S[:self.K]
        return S / np.maximum(np.sqrt((S * S).sum(1, keepdims=True)), 1e-300)


def map_chunk_host(hs: HostStream, E3: np.ndarray, info3: np.ndarray, F: int, delta_new: float = 1.0):
    """"mapping" of the module docstring for one chunk: E3 [3, d] fp32 unit rows, info3 [3, 4] -> (labels [3] int32, score [3] float64);
    hs.K, hs.S and hs.n are renewed.  Rows that are no candidates are never read."""
    cand = candidate_mask(info3)
    lng = cand & training_mask(info3, F)
    slots = np.flatnonzero(cand)
    labels, score = np.full(N_LOCAL, -1, np.int32), np.zeros(N_LOCAL)
    K0 = hs.K
    if K0 and slots.size:
        cos = np.asarray(E3)[slots].astype(np.float64) @ hs.centroids().T
        for s, row, k in zip(slots, cos, constrained_chunk(cos)):
            if k >= 0:
                labels[s], score[s] = k, row[k]
    for s in slots:
        k = int(labels[s])
        if K0 and lng[s] and k >= 0 and 1.0 - score[s] <= delta_new:
            hs.S[k] += np.asarray(E3[s], dtype=np.float64)
            hs.n[k] += 1
        elif lng[s] and hs.K < hs.capacity:
            labels[s], score[s] = hs.K, 1.0
            hs.S[hs.K], hs.n[hs.K] = np.asarray(E3[s], dtype=np.float64), 1
            hs.K += 1
    return labels, score


def emit_host(nc, cnt, act, K: int, max_speakers: Optional[int] = None):
    """nc [n], cnt [n], act [n, >= K] of n frames -> (count [n] uint8, speakers [n, 2] int32): diarize_host.reconstruct_host's last lines."""
    n = len(nc)
    count = np.where(nc > 0, np.minimum((2 * cnt + nc) // np.maximum(2 * nc, 1), _speaker_cap(max_speakers)), 0)
    a = np.asarray(act)[:, :K]
    order = np.argsort(-a, axis=1, kind="stable")[:, :2] if K else np.zeros((n, 0), np.int64)
    speakers = np.full((n, 2), -1, np.int32)
    for slot in range(min(2, K)):
        k = order[:, slot]
        ok = (count > slot) & (a[np.arange(n), k] > 0)
        speakers[ok, slot] = k[ok]
    return count.astype(np.uint8), speakers


def stitch_chunk_host(hs: HostStream, cls_row: np.ndarray, start: int, labels: np.ndarray, hold: int, max_speakers: Optional[int] = None,
                      n_end: Optional[int] = None):
    """"stitching" for one chunk: the ring takes the chunk's frames, the due frames leave -> (frame_lo, count [n] uint8, speakers [n, 2])."""
    cls_row = np.asarray(cls_row)
    F, q = len(cls_row), chunk_q(start)
    reach1 = F - q
    lo = max(hs.frontier, reach1 - RING)
    front1 = max(hs.frontier, reach1 - hold)
    if n_end:                                                              # the stream's last chunk: no frame beyond its end
        front1 = max(hs.frontier, min(front1, global_frames(n_end)))
    g = np.arange(lo, reach1)
    slot = g % RING
    fresh = g >= hs.reach
    hs.nc[slot[fresh]], hs.cnt[slot[fresh]], hs.act[slot[fresh]] = 0, 0, 0
    i = g + q
    m = (i >= 0) & (i < F)
    c = cls_row[i[m]]
    hs.nc[slot[m]] += 1
    hs.cnt[slot[m]] += _COUNT[c]
    on = _MASK[c]                                                          # [frames, 3]
    for k in {int(v) for v in labels if v >= 0}:
        hs.act[slot[m], k] += on[:, np.asarray(labels) == k].any(1)
    out = slot[:max(0, front1 - lo)]
    count, speakers = emit_host(hs.nc[out], hs.cnt[out], hs.act[out], hs.K, max_speakers)
    hs.frontier, hs.reach = max(front1, lo), max(hs.reach, reach1)
    return lo, count, speakers


def flush_host(hs: HostStream, n_samples: int, max_speakers: Optional[int] = None):
    """The end of the stream: every frame not yet emitted, up to global_frames(n_samples) -> (frame_lo, count, speakers)."""
    lo = hs.frontier
    hi = min(max(global_frames(n_samples), lo), lo + RING)
    g = np.arange(lo, hi)
    held = g < hs.reach
    slot = g % RING
    count, speakers = emit_host(np.where(held, hs.nc[slot], 0), np.where(held, hs.cnt[slot], 0), np.where(held[:, None], hs.act[slot], 0), hs.K,
                                max_speakers)
    hs.frontier = hi
    return lo, count, speakers


def step_host(hs: HostStream, E3, info3, cls_row, start: int, hold: int, delta_new: float = 1.0, max_speakers: Optional[int] = None,
              n_end: Optional[int] = None):
    """sdk_stream_step for one stream -> (labels [3], score [3], frame_lo, count, speakers)."""
    labels, score = map_chunk_host(hs, E3, info3, len(cls_row), delta_new)
    return (labels, score) + stitch_chunk_host(hs, cls_row, start, labels, hold, max_speakers, n_end)


def turns_of_frames(frame_lo: int, speakers: np.ndarray) -> List[Tuple[float, float, int]]:
    """speakers [n, 2] of the frames frame_lo .. -> (start_s, end_s, speaker) runs with segmentation.frames_to_ranges's boundaries, by start
    then speaker.  A turn that goes on in the next update ends at this update's last frame."""
    sp = np.asarray(speakers).reshape(-1, 2)
    out = []
    for k in sorted({int(v) for v in sp.reshape(-1) if v >= 0}):
        on = np.concatenate([[False], (sp == k).any(1), [False]])
        edge = np.flatnonzero(on[1:] != on[:-1])
        out += [((FRAME_HOP * (frame_lo + a) + 360) / SAMPLE_RATE, (FRAME_HOP * (frame_lo + b - 1) + 630) / SAMPLE_RATE, k) for a, b in zip(edge[::2], edge[1::2])]
    return sorted(out, key=lambda t: (t[0], t[2]))


# ------------------------------------------------------------------------------------------------ the bank
@dataclass
class StreamUpdate:
    frame_lo: int                             # the first newly emitted frame
    count: np.ndarray                         # [n] uint8 speakers per frame
    speakers: np.ndarray                      # [n, 2] int32, padded with -1

    def turns(self) -> List[Tuple[float, float, int]]:
        return turns_of_frames(self.frame_lo, self.speakers)


@dataclass
class _Slot:                                  # the host's side of one stream
    sched: ChunkSchedule
    base: int = 0                             # the stream sample at the head of its slot of the bank buffer
    frontier: int = 0                         # mirrors of the device's frontier and reach: integers of the schedule alone
    reach: int = 0
    pending: list = field(default_factory=list)
    starts: list = field(default_factory=list)
    labels: list = field(default_factory=list)
    scores: list = field(default_factory=list)
    info: list = field(default_factory=list)
    count: list = field(default_factory=list)
    speakers: list = field(default_factory=list)
    kept: list = field(default_factory=list)  # keep_embeddings: (E [3, d], cls [F]) per chunk
    K: int = 0


class StreamBank:
    """n_streams live streams on one Diarizer ("bank" in the module docstring).  push() feeds audio and returns what was newly emitted;
    finish(r) ends a stream and returns its DiarizationResult; reset(r) reopens the slot.  last_sync holds one dict per bank step of the last
    push or finish: {"downloads": 1, "uploads", "active"} - the one wait of a step is the download of its labels and emitted frames.
    keep_embeddings = True (a test hook) keeps every chunk's unit rows and class table in embeddings(r); they ride in the same download."""

    def __init__(self, diarizer, n_streams: int = 1, step_s: float = 0.5, latency_s: Optional[float] = None, capacity: int = 20,
                 delta_new: float = 1.0, max_speakers: Optional[int] = None):
        self.hop, self.latency, self.hold = check_stream_options(step_s, latency_s, capacity, delta_new, max_speakers)
        if not (isinstance(n_streams, (int, np.integer)) and 1 <= n_streams and n_streams * SLOT < (1 << 31)):
            raise ValueError(f"stream: n_streams={n_streams!r} (1 .. {((1 << 31) - 1) // SLOT}: the chunk starts inside the bank buffer are int32)")
        import torch
        self.dz, self.eng, self.R = diarizer, diarizer.eng, int(n_streams)
        self.step_s, self.capacity, self.delta_new, self.max_speakers = float(step_s), int(capacity), float(delta_new), max_speakers
        self.F, self.d = seg_frames(CHUNK), int(diarizer.resnet.cfg.embed_dim)
        self.state = self.eng.stream_state(self.R, self.capacity, self.d)
        self.buf = torch.zeros(self.R * SLOT, dtype=torch.int16, device=self.eng.device)
        dev = self.eng.device
        self._E = torch.zeros((N_LOCAL * self.R, self.d), dtype=torch.float32, device=dev)      # rows of streams without a chunk: never read
        self._info = torch.zeros((self.R, N_LOCAL, 4), dtype=torch.int32, device=dev)
        self._cls = torch.zeros((self.R, self.F), dtype=torch.uint8, device=dev)
        self._ns = torch.zeros(self.R, dtype=torch.int64, device=dev)                           # finish and reset mark their one stream here
        self._on = torch.zeros(self.R, dtype=torch.uint8, device=dev)
        self.slots = [_Slot(ChunkSchedule(self.hop)) for _ in range(self.R)]
        self.keep_embeddings = False
        self.last_sync: List[dict] = []

    # ---------------------------------------------------------------------------------------------- what a caller asks
    def due(self, r: int, n_new: int = 0) -> int:
        """How many chunks of stream r a push of n_new samples would process."""
        return self.slots[r].sched.due(n_new)

    def embeddings(self, r: int):
        """keep_embeddings: (E [C, 3, d] fp32, cls [C, F] uint8) of stream r's chunks so far."""
        kept = self.slots[r].kept
        if not kept:
            return np.zeros((0, N_LOCAL, self.d), np.float32), np.zeros((0, self.F), np.uint8)
        return np.stack([e for e, _ in kept]), np.stack([c for _, c in kept])

    def reset(self, r: int) -> None:
        self._on[r] = 1
        self.eng.stream_reset(self.state, self._on)
        self._on[r] = 0
        self.buf[r * SLOT:(r + 1) * SLOT].zero_()
        self.slots[r] = _Slot(ChunkSchedule(self.hop))

    def push(self, samples, logp=None) -> List[StreamUpdate]:
        """samples: one 16 kHz mono int16 array (or None) per stream.  logp: None, or per stream None or a [due(r, len), 589, 7] array that
        replaces the segmentation output of the stream's chunks that this push processes -> one StreamUpdate per stream.  The bank steps in
        the ResNet34's numerical contract; the engine's precision is what it was when the call returns, as after Diarizer.run in Backend."""
        prec = self.eng.precision
        try:
            return self._push(samples, logp)
        finally:
            if self.eng.precision != prec:
                self.eng.set_precision(prec)

    def _push(self, samples, logp):
        import torch
        if len(samples) != self.R or (logp is not None and len(logp) != self.R):
            raise ValueError(f"stream: push takes one array (or None) per stream ({self.R}), got {len(samples)}")
        xs = [np.zeros(0, np.int16) if x is None else np.ascontiguousarray(x, dtype=np.int16).reshape(-1) for x in samples]
        for r, x in enumerate(xs):
            if x.size and self.slots[r].sched.finished:
                raise ValueError(f"stream: push to stream {r}, which is finished (reset it first)")
        lps = [None] * self.R
        for r in range(self.R):
            lp = None if logp is None else logp[r]
            if lp is not None:
                n_due = self.due(r, xs[r].size)
                if tuple(lp.shape) != (n_due, self.F, 7):
                    raise ValueError(f"stream: stream {r}: injected logp must be [{n_due}, {self.F}, 7], got {tuple(lp.shape)}")
                lps[r] = torch.as_tensor(lp, dtype=torch.float32)
        self.last_sync = []
        out = [[] for _ in range(self.R)]
        fed, used = [0] * self.R, [0] * self.R
        while True:
            for r, x in enumerate(xs):                           # every sample crosses once, as room in the slot allows
                sl = self.slots[r]
                room = SLOT - (sl.sched.n - sl.base)
                k = min(room, x.size - fed[r])
                if k > 0:
                    o = r * SLOT + sl.sched.n - sl.base
                    self.buf[o:o + k] = torch.from_numpy(x[fed[r]:fed[r] + k]).to(self.eng.device, non_blocking=True)
                    sl.pending += sl.sched.push(k)
                    fed[r] += k
            while any(sl.pending for sl in self.slots):
                act = [r for r in range(self.R) if self.slots[r].pending]
                lp = None
                if any(lps[r] is not None for r in act):
                    if any(lps[r] is None for r in act):
                        raise ValueError("stream: logp must be given for every stream that has a chunk due, or for none")
                    lp = torch.stack([lps[r][used[r]] for r in act])
                    for r in act:
                        used[r] += 1
                self._bank_step(act, [self.slots[r].pending.pop(0) for r in act], lp, out)
            if all(fed[r] == xs[r].size for r in range(self.R)):
                break
            for r in range(self.R):                              # make room: the slot keeps its last chunk's worth
                self._compact(r)
        return [self._update(r, ups) for r, ups in enumerate(out)]

    def finish(self, r: int, logp=None) -> DiarizationResult:
        """The end of stream r: its last chunk when the grid chunks do not reach the end (logp [1, 589, 7] replaces its segmentation output),
        then every frame not yet emitted -> the DiarizationResult of everything emitted (cls is None).  The slot stays closed until reset."""
        prec = self.eng.precision
        try:
            return self._finish(r, logp)
        finally:
            if self.eng.precision != prec:
                self.eng.set_precision(prec)

    def _finish(self, r: int, logp):
        import torch
        sl = self.slots[r]
        if sl.sched.finished:
            raise ValueError(f"stream: stream {r} is finished already (reset it first)")
        self.last_sync = []
        out = [[] for _ in range(self.R)]
        n = sl.sched.n
        start = sl.sched.finish()
        if n == 0:
            return self.dz._empty()
        if start is not None:
            if n < CHUNK:                                        # the zero-padded chunk: nothing stale behind the samples
                self.buf[r * SLOT + n:r * SLOT + CHUNK].zero_()
            lp = None if logp is None else torch.as_tensor(logp, dtype=torch.float32).reshape(1, self.F, 7)
            self._bank_step([r], [start], lp, out, n_end=n)
        self._ns[r], self._on[r] = n, 1                          # two scalars: nothing as long as the bank crosses for one stream's end
        st = self.eng.stream_flush(self.state, self._ns, self._on, self.max_speakers)
        self._ns[r], self._on[r] = 0, 0
        G = global_frames(n)
        m = max(0, G - sl.frontier)
        cent, _, _ = self.eng.stream_centroids(self.state, r, 1)
        parts = [st.emit_lo[r:r + 1], st.emit_n[r:r + 1], st.count[r, :m], st.speakers[r, :m], cent[0, :sl.K]]
        host = _download(parts)
        self.last_sync.append({"downloads": 1, "uploads": 0, "active": 1})
        if int(host[0][0]) != sl.frontier or int(host[1][0]) != m:
            raise RuntimeError(f"stream: stream {r}: the device flushed frames {int(host[0][0])} + {int(host[1][0])}, the schedule says {sl.frontier} + {m}")
        sl.count.append(host[2])
        sl.speakers.append(host[3].reshape(-1, 2))
        sl.frontier = G
        count = np.concatenate(sl.count) if sl.count else np.zeros(0, np.uint8)
        speakers = np.concatenate(sl.speakers) if sl.speakers else np.full((0, 2), -1, np.int32)
        C = len(sl.starts)
        return DiarizationResult(turns_from_frames(speakers, sl.K), sl.K, host[4].reshape(sl.K, self.d).copy(),
                                 np.asarray(sl.labels, np.int32).reshape(C, N_LOCAL), count, speakers, np.asarray(sl.starts, np.int64),
                                 np.asarray(sl.info, np.int32).reshape(C, N_LOCAL, 4), None, np.asarray(sl.scores, np.float32).reshape(C, N_LOCAL))

    # ---------------------------------------------------------------------------------------------- inside
    def _compact(self, r: int) -> None:
        """Move what stream r still needs - from its next chunk's start, and never less than the last chunk's worth - to the head of its slot."""
        sl = self.slots[r]
        keep = max(sl.base, min(sl.sched.done * self.hop, sl.sched.n - CHUNK))
        if keep > sl.base:
            a, b = r * SLOT + keep - sl.base, r * SLOT + sl.sched.n - sl.base
            self.buf[r * SLOT:r * SLOT + b - a] = self.buf[a:b].clone()
            sl.base = keep

    def _update(self, r: int, ups) -> StreamUpdate:
        if not ups:
            return StreamUpdate(self.slots[r].frontier, np.zeros(0, np.uint8), np.full((0, 2), -1, np.int32))
        return StreamUpdate(ups[0][0], np.concatenate([u[1] for u in ups]), np.concatenate([u[2] for u in ups]))

    def _bank_step(self, act: List[int], starts: List[int], lp, out, n_end: int = 0) -> None:
        """One bank step: the chunks starts[i] of the streams act[i].  n_end: finish()'s chunk, the stream ends at that sample."""
        import torch
        eng, R, B = self.eng, self.R, len(act)
        sync = {"downloads": 0, "uploads": 1, "active": B}
        if eng.precision != self.dz.resnet.precision:
            eng.set_precision(self.dz.resnet.precision)          # the front end's output format follows the embedding's numerical contract
        abs_start, on, end = np.zeros(R, np.int64), np.zeros(R, np.int64), np.zeros(R, np.int64)
        abs_start[act], on[act], end[act] = starts, 1, n_end
        in_buf = [r * SLOT + s - self.slots[r].base for r, s in zip(act, starts)]
        up = torch.from_numpy(np.concatenate([abs_start, on, end, np.asarray(act, np.int64), np.asarray(in_buf, np.int64)])).to(eng.device)
        starts_dev, on_dev, end_dev = up[:R], up[R:2 * R].to(torch.uint8), up[2 * R:3 * R]
        idx, cut = up[3 * R:3 * R + B], up[3 * R + B:].to(torch.int32)
        if lp is not None:
            lp = lp.to(eng.device)
            sync["uploads"] += 1
        cls, info, E = self.dz.embed_chunks(self.buf, int(self.buf.numel()), cut, lp)
        if B == R:                                               # every stream steps: the batch is the bank, in order
            cls_r, info_r, E_r = cls, info, E
        else:                                                    # the batch's rows go to their streams' places
            self._cls.index_copy_(0, idx, cls)
            self._info.index_copy_(0, idx, info)
            self._E.view(R, N_LOCAL, self.d).index_copy_(0, idx, E.view(B, N_LOCAL, self.d))
            cls_r, info_r, E_r = self._cls, self._info, self._E
        st = eng.stream_step(self.state, E_r.contiguous(), info_r.contiguous(), cls_r.contiguous(), starts_dev, on_dev, self.hop, self.latency,
                             self.delta_new, self.max_speakers, end_dev if n_end else None)
        emit = []                                                # what every stream emits follows from its chunk starts alone
        for r, s in zip(act, starts):
            sl = self.slots[r]
            reach1 = self.F - chunk_q(s)
            lo = max(sl.frontier, reach1 - RING)
            front1 = max(sl.frontier, reach1 - self.hold)
            if n_end:
                front1 = max(sl.frontier, min(front1, global_frames(n_end)))
            emit.append((lo, max(0, front1 - lo)))
            sl.frontier, sl.reach = max(front1, lo), max(sl.reach, reach1)
        M = max(n for _, n in emit)
        parts = [st.labels, st.score, st.K, st.emit_lo, st.emit_n, info_r, st.count[:, :M], st.speakers[:, :M]]
        if self.keep_embeddings:
            parts += [E_r, cls_r]
        host = _download(parts)                                  # the step's one wait
        sync["downloads"] += 1
        self.last_sync.append(sync)
        labels, score, K, e_lo, e_n, info_h = host[0].reshape(R, 3), host[1].reshape(R, 3), host[2], host[3], host[4], host[5].reshape(R, 3, 4)
        count, speakers = host[6].reshape(R, M), host[7].reshape(R, M, 2)
        for (r, s), (lo, n) in zip(zip(act, starts), emit):
            sl = self.slots[r]
            if int(e_lo[r]) != lo or int(e_n[r]) != n:
                raise RuntimeError(f"stream: stream {r}: the device emitted frames {int(e_lo[r])} + {int(e_n[r])}, the schedule says {lo} + {n}")
            sl.starts.append(s)
            sl.labels.append(labels[r].copy())
            sl.scores.append(score[r].copy())
            sl.info.append(info_h[r].copy())
            sl.K = int(K[r])
            sl.count.append(count[r, :n].copy())
            sl.speakers.append(speakers[r, :n].copy())
            if self.keep_embeddings:
                sl.kept.append((host[8].reshape(R, N_LOCAL, self.d)[r].copy(), host[9].reshape(R, self.F)[r].copy()))
            out[r].append((lo, sl.count[-1], sl.speakers[-1]))


def _download(parts):
    """Device tensors of any dtype -> their numpy arrays (flat), through ONE device-to-host copy."""
    import torch
    flat = [p.contiguous().view(-1).view(torch.uint8) for p in parts]
    host = torch.cat(flat).cpu().numpy()
    out, o = [], 0
    for p, f in zip(parts, flat):
        n = int(f.numel())
        out.append(host[o:o + n].view(_NP[str(p.dtype)]).copy())
        o += n
    return out


_NP = {"torch.int32": np.int32, "torch.int64": np.int64, "torch.float32": np.float32, "torch.uint8": np.uint8}
