"""The streaming rule of stream.py's docstring, written a second time from the text alone: no ring (every frame of the stream keeps its row),
the constrained assignment by enumerating EVERY one-to-one map of candidates to speakers (not the three best per row), and the emission
frontier as a plain integer.  It also measures how far every decision of a run stands from its threshold (`margin`), so a test can refuse
inputs that float64 rounding could decide either way."""
from __future__ import annotations

import itertools

import numpy as np

F_HOP, CHUNK = 270, 160000
SPEAKERS_OF = [(), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2)]


def frames_of(n_samples: int) -> int:
    return max(0, -(-(int(n_samples) - 495) // F_HOP))


def schedule(n: int, hop: int):
    """The chunk starts of a stream of n samples: the grid chunks that fit, then what finish() adds."""
    if n == 0:
        return []
    if n <= CHUNK:
        return [0]
    st = list(range(0, n - CHUNK + 1, hop))
    if (n - CHUNK) % hop:
        st.append(n - CHUNK)
    return st


def best_map(cos: np.ndarray):
    """cos [m, K] -> (labels of the m candidates, gap between the best total and the next valid one; inf when there is no other).
    min(m, K) candidates get pairwise different speakers, the others -1; largest total summed in slot order; ties to the smallest label
    tuple with -1 after every speaker."""
    m, K = cos.shape
    n = min(m, K)
    if K >= m and m == 3:                                                 # all K^3 triples at once; C order is the tie order
        tot = (cos[0][:, None, None] + cos[1][None, :, None]) + cos[2][None, None, :]
        i = np.arange(K)
        bad = (i[:, None, None] == i[None, :, None]) | (i[:, None, None] == i[None, None, :]) | (i[None, :, None] == i[None, None, :])
        tot = np.where(bad, -np.inf, tot).reshape(-1)
        b = int(np.argmax(tot))
        rest = np.delete(tot, b)
        gap = float(tot[b] - rest.max()) if rest.size and np.isfinite(rest.max()) else np.inf
        return tuple(int(v) for v in np.unravel_index(b, (K, K, K))), gap
    cands = []
    for lab in itertools.product(*[list(range(K)) + [-1]] * m):
        used = [k for k in lab if k >= 0]
        if len(used) != n or len(set(used)) != n:
            continue
        tot = 0.0
        for i, k in enumerate(lab):
            if k >= 0:
                tot = tot + cos[i, k]
        cands.append((-tot, tuple(k if k >= 0 else K for k in lab), lab))
    cands.sort()
    gap = cands[1][0] - cands[0][0] if len(cands) > 1 else np.inf
    return cands[0][2], float(gap)


class RefStream:
    def __init__(self, capacity: int, d: int, hop: int, latency: int, delta_new: float = 1.0, max_speakers=None, F: int = 589):
        self.cap, self.d, self.hop, self.delta, self.F = capacity, d, hop, float(delta_new), F
        self.hold = (latency - hop) // F_HOP
        self.per_frame = 2 if max_speakers is None else min(2, int(max_speakers))
        self.sums, self.n = [], []                                        # one float64 row and one count per speaker, in founding order
        self.act = np.zeros((0, capacity), np.int64)                      # per frame of the stream
        self.nc, self.total = np.zeros(0, np.int64), np.zeros(0, np.int64)
        self.emitted = 0
        self.margin = np.inf                                              # the least distance of any decision from its threshold

    @property
    def K(self):
        return len(self.sums)

    def _grow(self, G):
        if G > len(self.nc):
            add = G - len(self.nc)
            self.act = np.concatenate([self.act, np.zeros((add, self.cap), np.int64)])
            self.nc, self.total = np.concatenate([self.nc, np.zeros(add, np.int64)]), np.concatenate([self.total, np.zeros(add, np.int64)])

    def _emit(self, upto):
        lo, hi = self.emitted, max(self.emitted, upto)
        self._grow(hi)
        count, speakers = np.zeros(hi - lo, np.uint8), np.full((hi - lo, 2), -1, np.int32)
        for j, g in enumerate(range(lo, hi)):
            if self.nc[g]:
                count[j] = min((2 * self.total[g] + self.nc[g]) // (2 * self.nc[g]), self.per_frame)
            ranked = sorted((k for k in range(self.K) if self.act[g, k] > 0), key=lambda k: (-self.act[g, k], k))
            for s in range(min(int(count[j]), len(ranked), 2)):
                speakers[j, s] = ranked[s]
        self.emitted = hi
        return lo, count, speakers

    def step(self, E3, info3, cls_row, start, n_end=None):
        """-> (labels [3], score [3], frame_lo, count, speakers).  n_end: the chunk is the one finish() adds to a stream of n_end samples."""
        F = self.F
        info3 = np.asarray(info3)
        cand = [s for s in range(3) if info3[s, 3] != 0 and info3[s, 0] > 0]
        is_long = {s: 5 * int(info3[s, 1]) >= F for s in cand}
        labels, score = [-1, -1, -1], [0.0, 0.0, 0.0]
        K0 = self.K
        if K0 and cand:
            U = np.stack([v / np.sqrt(np.dot(v, v)) for v in self.sums])
            cos = np.stack([U @ np.asarray(E3[s], np.float64) for s in cand])
            lab, gap = best_map(cos)
            self.margin = min(self.margin, gap)
            for i, s in enumerate(cand):
                if lab[i] >= 0:
                    labels[s], score[s] = lab[i], float(cos[i, lab[i]])
                    self.margin = min(self.margin, abs(1.0 - cos[i, lab[i]] - self.delta))
        for s in cand:
            k = labels[s]
            matched = K0 > 0 and k >= 0 and 1.0 - score[s] <= self.delta
            if is_long[s] and matched:
                self.sums[k] = self.sums[k] + np.asarray(E3[s], np.float64)
                self.n[k] += 1
            elif is_long[s] and self.K < self.cap:
                labels[s], score[s] = self.K, 1.0
                self.sums.append(np.asarray(E3[s], np.float64).copy())
                self.n.append(1)
        q = (135 - int(start)) // F_HOP
        self._grow(F - q)
        for i in range(F):
            g = i - q
            if g < self.emitted or g < 0:
                continue                                                  # emitted frames never change
            who = SPEAKERS_OF[int(cls_row[i])]
            self.nc[g] += 1
            self.total[g] += len(who)
            for k in {labels[s] for s in who if labels[s] >= 0}:
                self.act[g, k] += 1
        return (np.asarray(labels, np.int32), np.asarray(score)) + self._emit(F - q - self.hold if n_end is None else min(F - q - self.hold, frames_of(n_end)))

    def flush(self, n_samples):
        return self._emit(frames_of(n_samples))


def run_stream(E, info, cls, starts, n_samples, capacity, hop, latency, delta_new=1.0, max_speakers=None):
    """A whole stream: E [C, 3, d], info [C, 3, 4], cls [C, F], starts [C] -> dict of labels [C, 3], score, count [G], speakers [G, 2], K, ref, and
    what every step and then the flush emitted: lows [C + 1] (the first frame) and ns [C + 1] (how many)."""
    ref = RefStream(capacity, E.shape[2], hop, latency, delta_new, max_speakers, cls.shape[1])
    labels, score, count, speakers, lows = [], [], [], [], []
    for c in range(len(starts)):
        added = c == len(starts) - 1 and (n_samples < CHUNK or (n_samples - CHUNK) % hop != 0)          # the chunk finish() adds
        lab, sc, lo, cnt, spk = ref.step(E[c], info[c], cls[c], int(starts[c]), n_samples if added else None)
        labels.append(lab), score.append(sc), count.append(cnt), speakers.append(spk), lows.append(int(lo))
    lo, cnt, spk = ref.flush(n_samples)
    count.append(cnt), speakers.append(spk), lows.append(int(lo))
    return {"labels": np.asarray(labels, np.int32).reshape(-1, 3), "score": np.asarray(score).reshape(-1, 3), "count": np.concatenate(count),
            "speakers": np.concatenate(speakers), "K": ref.K, "ref": ref, "lows": lows, "ns": [len(v) for v in count]}


def second_column_weight(name: str, s: dict, n_samples: int, ref: dict, capacity, hop, latency, delta_new=1.0, score_bound: float = 1e-6) -> float:
    """partial_width.weight for a stream wider than 256 columns: the run without the columns 256.. of its rows against `ref` (the run on the full
    rows) - labels, frames and the speaker count as integers, the scores and the speakers' sums against score_bound."""
    import partial_width as PW
    cut = run_stream(PW.first_columns(s["E"]), s["info"], s["cls"], s["starts"], n_samples, capacity, hop, latency, delta_new)
    sums = [(np.stack(r["ref"].sums) if r["K"] else np.zeros((0, s["E"].shape[2]))) for r in (ref, cut)]
    return PW.weight(name, ints=[(ref[q], cut[q]) for q in ("labels", "count", "speakers", "K")], floats=[(ref["score"], cut["score"]), tuple(sums)],
                     bound=score_bound)


def make_stream(seed: int, d: int, n: int, hop: int, n_speakers: int = 5, noise: float = 0.35):
    """A generated stream of n samples: per chunk of schedule(n, hop) a random class table (runs of silence, single speakers and overlap),
    its info (diarize.masks_host) and three unit rows drawn around n_speakers seeded unit centres (oracle.spectral.vmf_mixture); the local
    speakers of a chunk are different people -> dict of E [C, 3, d] fp32, info [C, 3, 4], cls [C, F] uint8, starts [C] int64."""
    import importlib
    from oracle.spectral import vmf_mixture
    masks_host = importlib.import_module("speaker-diarization-toolkit_amd.diarize").masks_host
    rng = np.random.default_rng(seed)
    starts = np.asarray(schedule(n, hop), np.int64)
    C, F = len(starts), 589
    cls = np.zeros((C, F), np.uint8)
    for c in range(C):
        i = 0
        while i < F:
            m = int(rng.integers(1, 90))
            cls[c, i:i + m] = 0 if rng.random() < 0.3 else rng.integers(1, 7)
            i += m
    if C > 2:
        cls[1] = 0                                                        # a silent chunk: no candidate
        cls[2, :] = np.where(np.arange(F) < 60, 1, 0)                     # a short candidate: 60 clean frames
    pool, who = vmf_mixture(40 * n_speakers + 3 * C, d, n_speakers, seed, noise)
    E = np.zeros((C, 3, d), np.float32)
    used = np.zeros(len(pool), bool)
    for c in range(C):
        for s, k in enumerate(rng.permutation(n_speakers)[:3] if n_speakers >= 3 else rng.integers(0, n_speakers, 3)):
            j = int(np.flatnonzero((who == k) & ~used)[0])
            used[j] = True
            E[c, s] = pool[j]
    return {"E": E, "info": masks_host(cls, 126)[1], "cls": cls, "starts": starts}
