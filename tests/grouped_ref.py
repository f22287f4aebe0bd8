"""Case builders for the grouped (many-recordings) diarization kernels of csrc/diarize.hip at their group, lane and block edges.  Builders
only: the arbiters are tests/diarize_ref.py, tests/assign_ref.py, cluster.fold_small_clusters and the package's host restatements.  The CPU
twin (test_diarize_grouped_edges_cpu.py) checks every fixture condition on the references alone; the GPU file runs the same cases."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assign_ref as AR  # noqa: E402
import diarize_ref as DR  # noqa: E402
from conftest import sub  # noqa: E402

dz = sub("diarize")
seg = sub("segmentation")
cluster = sub("cluster")
F, HOP, RATE = 589, 270, 16000
I32_MAX = int(np.iinfo(np.int32).max)


def offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def samples_for(G: int) -> int:
    """The least sample count with G global frames (0 frames: a recording too short for any)."""
    return 300 if G == 0 else 495 + HOP * (G - 1) + 1


# ------------------------------------------------------------------------------------------------ group tables
def group_tables():
    """name -> elements per group.  The elements are chunks, frames, clusters or recordings, whatever the kernel's table counts."""
    rng = np.random.default_rng(300)
    return {"R1": [37],
            "R7_empty_first_last_twice": [0, 5, 0, 0, 9, 3, 0],
            "boundary_64_256": [64, 192, 7],                               # offsets 0, 64, 256, 263
            "boundary_255_257": [255, 2, 30],                              # offsets 0, 255, 257, 287
            "R300": rng.integers(1, 4, 300).tolist()}


def table_classes(counts):
    """The shape classes a table of counts enters (asserted present by the CPU twin)."""
    off, c = offsets(counts), np.asarray(counts)
    return dict(R=len(c), empty_first=bool(c[0] == 0), empty_last=bool(c[-1] == 0), two_empty=bool(((c[:-1] == 0) & (c[1:] == 0)).any()),
                at_64=bool(64 in off[1:-1]), at_256=bool(256 in off[1:-1]), at_255=bool(255 in off[1:-1]), at_257=bool(257 in off[1:-1]),
                second_block=bool(len(c) > 256))


# ------------------------------------------------------------------------------------------------ reconstruct
def seeing(starts, G):
    """-> per global frame the (chunk, frame in chunk) pairs that see it, chunks ascending."""
    q = [(135 - int(s)) // HOP for s in starts]
    return [[(c, g + q[c]) for c in range(len(starts)) if 0 <= g + q[c] < F] for g in range(G)]


def mean_counts(cls, starts, G):
    """-> (cnt [G], nc [G]): the speakers summed over the chunks that see a frame, and those chunks' number (the fixture conditions read them)."""
    cnt, nc = np.zeros(G, np.int64), np.zeros(G, np.int64)
    for g, see in enumerate(seeing(starts, G)):
        nc[g] = len(see)
        cnt[g] = sum(len(DR.CLASSES[cls[c, i]]) for c, i in see)
    return cnt, nc


def random_cls(rng, Cn, p_sil=0.3):
    cls = np.zeros((Cn, F), np.uint8)
    for c in range(Cn):
        i = 0
        while i < F:
            n = int(rng.integers(1, 90))
            cls[c, i:i + n] = 0 if rng.random() < p_sil else rng.integers(1, 7)
            i += n
    return cls


def pack_of(recs):
    """recs: list of dict(n, starts, cls, labels, K) -> the pack's tables."""
    return dict(n=np.array([r["n"] for r in recs], np.int64), starts=[r["starts"] for r in recs], cls=np.concatenate([r["cls"] for r in recs]),
                labels=np.concatenate([r["labels"] for r in recs]).astype(np.int32), chunk_off=offsets([len(r["starts"]) for r in recs]),
                frame_off=offsets([dz.global_frames(r["n"]) for r in recs]), cent_off=offsets([r["K"] for r in recs]),
                K_list=[r["K"] for r in recs], planted=[r.get("planted", {}) for r in recs])


def random_recording(rng, n, K, step_s, hi=None):
    """Random classes; labels in [-1, hi) (hi = K by default; above K: labels that name no cluster)."""
    st = seg.chunk_starts(n, step_s)
    hi = max(K, 1) if hi is None else hi
    lab = rng.integers(-1, hi, (len(st), 3)) if K or hi > 1 else np.full((len(st), 3), -1)
    return dict(n=n, starts=st, cls=random_cls(rng, len(st)), labels=lab.astype(np.int32), K=K)


def reconstruct_edges(step_s, seed=21):
    """G_r in {257, 1, 255, 256, 0, 40} with K_r in {0, 1, 64, 65, 3, 200} (one chunk each: the recordings are below 10 s), and a 25-s
    recording whose inner frames are seen by about 10 / step_s chunks."""
    rng = np.random.default_rng(seed)
    recs = [random_recording(rng, samples_for(G), K, step_s) for G, K in [(257, 0), (1, 1), (255, 64), (256, 65), (0, 3), (40, 200)]]
    recs.append(random_recording(rng, 25 * RATE + 77, 5, step_s))
    return pack_of(recs)


def constructed_recording(rng, step_s):
    """20 s, K = 3.  Chunk labels are (1, 0, 2) but for the last two chunks: (2, 2, 0), a label repeated inside a chunk, and (3, 0, 8), labels
    equal to K and K + 5.  Planted in frames 100 .. 430, which those two chunks do not see: frames with a mean count of exactly 0.5 and 1.5,
    two clusters tied in act (local speakers 0 and 1 carry clusters 1 and 0, so the lower CLUSTER must take slot 0) and three tied."""
    n, K = 20 * RATE, 3
    st = seg.chunk_starts(n, step_s)
    Cn, G = len(st), dz.global_frames(n)
    cls = random_cls(rng, Cn)
    labels = np.tile(np.array([1, 0, 2], np.int32), (Cn, 1))
    labels[-2], labels[-1] = (2, 2, 0), (K, 0, K + 5)
    see = seeing(st, G)
    planted = {"half": [], "one_and_half": [], "tie2": [], "tie3": []}
    for g in range(100, 430):
        s, nc = see[g], len(see[g])
        assert all(c < Cn - 2 for c, _ in s)
        kind = ("half", "one_and_half", "tie2", "tie3", None)[g % 5]
        if kind in ("half", "one_and_half") and nc % 2:
            continue
        if kind == "tie3" and (nc < 3 or 4 * (nc // 3) < nc):            # the chunks past a multiple of 3 are silent: keep the mean count at 1.5 or more
            continue
        for j, (c, i) in enumerate(s):
            if kind == "half":
                cls[c, i] = 1 if j < nc // 2 else 0
            elif kind == "one_and_half":
                cls[c, i] = 4 if j < nc // 2 else 1
            elif kind == "tie2":
                cls[c, i] = 4
            elif kind == "tie3":
                cls[c, i] = (4, 5, 6)[j % 3] if j < 3 * (nc // 3) else 0
        if kind:
            planted[kind].append(g)
    return dict(n=n, starts=st, cls=cls, labels=labels, K=K, planted=planted)


def reconstruct_constructed(step_s, seed=22):
    """The constructed recording, one whose labels are all -1, one with random labels up to K_r + 5, and one too short for a frame."""
    rng = np.random.default_rng(seed)
    none = random_recording(rng, 12 * RATE + 5, 2, step_s)
    none["labels"][:] = -1
    return pack_of([constructed_recording(rng, step_s), none, random_recording(rng, 300, 2, step_s),
                    random_recording(rng, 12 * RATE + 131, 4, step_s, hi=4 + 6)])


def reconstruct_tables(counts, seed=23):
    """One recording per group with counts[r] frames (a single chunk each) and K_r in 0 .. 3."""
    rng = np.random.default_rng(seed)
    return pack_of([random_recording(rng, samples_for(int(G)), int(rng.integers(0, 4)), 1.0) for G in counts])


# ------------------------------------------------------------------------------------------------ assign
ASSIGN_SEED = {64: 1, 512: 1}    # the CPU twin asserts that the reference alone keeps >= 95 % of the chunks with these


def assign_edges(d, seed):
    """Groups {empty, K_r = 64, K_r = 65, K_r = 300, empty}: the first without chunks or clusters, the last with clusters and no chunks ->
    (E, info, cent64, chunk_off, cent_off, per-recording (E_r, info_r, cent_r))."""
    none = (np.zeros((0, d), np.float32), np.zeros((0, 3, 4), np.int32), np.zeros((0, d)))
    per = [none]
    for n, K in enumerate((64, 65, 300)):
        E, info, tr, tl = AR.make_case(seed * 1000 + n, 24, K, d=d, train_per_cluster=1)
        per.append((E, info, AR.centroids(E, info, tr, tl)))
    c = np.random.default_rng(seed).standard_normal((2, d))
    per.append((none[0], none[1], c / np.linalg.norm(c, axis=1, keepdims=True)))
    return (np.concatenate([p[0] for p in per]), np.concatenate([p[1] for p in per]), np.concatenate([p[2] for p in per]),
            offsets([p[1].shape[0] for p in per]), offsets([p[2].shape[0] for p in per]), per)


# ------------------------------------------------------------------------------------------------ fold
def fold_recording(rng, sizes, mcs, d, plant=None):
    """Unit rows around K well-separated centres with canonical labels (test_diarize_many_cpu.fold_cases' recipe).  plant {small: large}:
    the small cluster's centre lies next to that large cluster's -> (E float64 [N, d], labels int32, min_cluster_size)."""
    K = len(sizes)
    centres = rng.standard_normal((K, d))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    for s, t in (plant or {}).items():
        v = rng.standard_normal(d)
        centres[s] = centres[t] + 0.15 * v / np.linalg.norm(v)
        centres[s] /= np.linalg.norm(centres[s])
    lab = np.concatenate([np.arange(K), rng.permutation(np.repeat(np.arange(K), np.asarray(sizes) - 1))])
    E = centres[lab] + 0.3 * rng.standard_normal((len(lab), d)) / np.sqrt(d)
    E = (E / np.linalg.norm(E, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    assert np.array_equal(cluster.canonical_labels(lab), lab)
    return E, lab.astype(np.int32), mcs


PLANT = {5: 3, 70: 66, 100: 127, 131: 129, 134: 130, 135: 63}    # small -> its best large cluster: below 64, in 64 .. 127, at or above 128


def fold_edges(d, seed=31):
    """[all clusters large, 130 large and 6 small (sizes exactly eff and eff - 1; the small ones' best large clusters planted by PLANT), no
    large cluster, one cluster] -> list of (E, labels, min_cluster_size) for test_diarize_many_cpu.fold_tables."""
    rng = np.random.default_rng(seed)
    big = [3] * 136
    for s in PLANT:
        big[s] = 2
    return [fold_recording(rng, [6, 7, 9], 4, d), fold_recording(rng, big, 3, d, PLANT), fold_recording(rng, [2] * 15, 7, d),
            fold_recording(rng, [3], 2, d)]


def fold_many(d, seed=32):
    """R = 300 recordings of 1 - 3 clusters; with 15 - 20 rows each the effective minimum is 2, so the clusters of one row fold."""
    rng = np.random.default_rng(seed)
    shapes = [[15], [14, 1], [1, 19], [9, 8, 1], [10, 1, 9], [1, 1, 16], [7, 8]]
    return [fold_recording(rng, shapes[int(rng.integers(0, len(shapes)))], 3, d) for _ in range(300)]


def fold_tables_case(counts, d=64, seed=34):
    """Groups of counts[r] clusters (None for an empty group): random unit centres, a cluster of 15 equal rows (large) or of one row (small
    wherever the recording's effective minimum reaches 2)."""
    rng = np.random.default_rng(seed)
    cases = []
    for K in counts:
        if not K:
            cases.append(None)
            continue
        c = rng.standard_normal((int(K), d))
        c = (c / np.linalg.norm(c, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
        sizes = np.where(rng.random(int(K)) < 0.5, 15, 1)
        cases.append((np.repeat(c, sizes, axis=0), np.repeat(np.arange(int(K)), sizes).astype(np.int32), 2))
    return cases


def fold_pack(cases, fold_tables):
    """test_diarize_many_cpu.fold_tables over the recordings that have clusters, the empty groups (None) put back into the tables."""
    cent, sizes, cl_off, eff, cent_off, ref, margins = fold_tables([c for c in cases if c is not None])
    n_cl, n_kept, eff, ref = np.diff(cl_off).tolist(), np.diff(cent_off).tolist(), eff.tolist(), list(ref)
    full = [(0, 0, 1, None) if c is None else (n_cl.pop(0), n_kept.pop(0), eff.pop(0), ref.pop(0)) for c in cases]
    return cent, sizes, offsets([f[0] for f in full]), np.array([f[2] for f in full]), offsets([f[1] for f in full]), [f[3] for f in full], margins


def _unit(d, entries):
    v = np.zeros(d)
    for i, x in entries:
        v[i] = x
    return v


def fold_exact(d):
    """Hand-written centroids whose fma chains are exact: entries from {+-0.5, +-1}, unit length.  Every recording holds 2 small clusters
    FIRST (so the first large cluster is not the recording's first), then 130 large ones.  The small clusters are (0.5, 0.5, 0.5, 0.5) on the
    columns 0, 1, d - 2, d - 1 and its negative; the large ones are basis vectors e_a with 4 <= a < d - 2 (cosine 0), but for those planted:
      u = e_0, v = 0.5 (e_1 + e_{d-1}) - 0.5 (e_7 + e_9): cosine +0.5 with the first small cluster, bit for bit, by two different chains.
    Recordings: tie at large j, j + 1 as (u, v) and (v, u); at j, j + 64 as (u, v) and (v, u); one NaN in the otherwise best large centroid
    (the small cluster itself with a NaN in a zero column); a NaN in every large centroid.
    -> (cent64, sizes, cl_off, eff, cent_off, expected target [Kc], names).  The second small cluster (the negative) meets cosine -0.5 at the
    planted pair and 0 elsewhere: its target is the first large cluster with cosine 0."""
    u = _unit(d, [(0, 1.0)])
    v = _unit(d, [(1, 0.5), (d - 1, 0.5), (7, -0.5), (9, -0.5)])
    s0 = _unit(d, [(0, 0.5), (1, 0.5), (d - 2, 0.5), (d - 1, 0.5)])
    nL, nS = 130, 2
    cents, target, names = [], [], []
    cols = [4 + (i % (d - 6 - 4)) for i in range(nL)]                     # basis columns away from 0, 1, 3 (the NaN column), d - 2, d - 1
    cols = [c if c not in (7, 9) else c + 20 for c in cols]               # and from v's columns 7 and 9

    def recording(planted, nan_all=False):
        large = np.stack([_unit(d, [(c, 1.0)]) for c in cols])
        for j, w in planted.items():
            large[j] = w
        if nan_all:
            large[:, 3] = np.nan
        return np.concatenate([np.stack([s0, -s0]), large])

    j = 37
    for name, a, b2 in [("lanes_uv", (j, u), (j + 1, v)), ("lanes_vu", (j, v), (j + 1, u)), ("same_lane_uv", (j, u), (j + 64, v)),
                        ("same_lane_vu", (j, v), (j + 64, u))]:
        planted = {a[0]: a[1], b2[0]: b2[1]}
        cents.append(recording(planted))
        first_zero = min(i for i in range(nL) if i not in planted)
        target.append([nS + j, nS + first_zero] + list(range(nS, nS + nL)))
        names.append(name)
    best_nan = s0.copy()
    best_nan[3] = np.nan
    cents.append(recording({5: best_nan, 90: u, 91: v}))                   # the NaN cluster (cosine 1 but for the NaN) is never chosen: 90 ties 91
    target.append([nS + 90, nS + 0] + list(range(nS, nS + nL)))
    names.append("one_nan")
    cents.append(recording({90: u}, nan_all=True))                        # every cosine NaN: the first large cluster, not the recording's first
    target.append([nS, nS] + list(range(nS, nS + nL)))
    names.append("all_nan")
    K = nS + nL
    R = len(cents)
    sizes = np.tile(np.array([1] * nS + [2] * nL), R)
    cl_off = offsets([K] * R)
    target = np.concatenate([np.asarray(t) + int(cl_off[r]) for r, t in enumerate(target)]).astype(np.int32)
    return np.concatenate(cents), sizes, cl_off, np.full(R, 2), offsets([nL] * R), target, names


def number_kept(target, cl_off, cent_off):
    """A hand-written target vector -> remap: the kept clusters of a recording numbered from cent_off[r] by the lowest cluster sent to them."""
    remap = np.full(len(target), -1, np.int32)
    for r in range(len(cl_off) - 1):
        new = {}
        for j in range(int(cl_off[r]), int(cl_off[r + 1])):
            remap[j] = new.setdefault(int(target[j]), int(cent_off[r]) + len(new))
    return remap


def chain(a, b):
    """sum a_i b_i in column order, one product and one sum per step (exact inputs: equal to the kernel's fma chain)."""
    acc = 0.0
    for x, y in zip(a, b):
        acc = acc + x * y
    return acc


def cut_for(Kc, n, seed=33):
    """n entries in [0, Kc) with -1 and Kc among them."""
    c = np.random.default_rng(seed).integers(0, max(Kc, 1), n).astype(np.int32)
    if n >= 4:
        c[1], c[n - 2], c[n // 2] = -1, Kc, Kc + 7
    return c


# ------------------------------------------------------------------------------------------------ first seen / renumber
def speakers_edges(seed=41):
    """-> (speakers per recording, frame_off, cent_off, names)."""
    rng = np.random.default_rng(seed)

    def scattered(K, G):                                                   # about half of the clusters never surface
        sp = np.full((G, 2), -1, np.int32)
        seen = rng.permutation(K)[:K // 2]
        for g in range(G):
            if rng.random() < 0.8:
                sp[g, 0] = seen[int(rng.integers(0, len(seen)))]
                if rng.random() < 0.5:
                    k = seen[int(rng.integers(0, len(seen)))]
                    sp[g, 1] = k if k != sp[g, 0] else -1
        return sp
    both = np.full((30, 2), -1, np.int32)
    both[3], both[7], both[9], both[12] = (2, 1), (2, 0), (4, 9), (1, 2)   # two new at once; slot 0 old and slot 1 new; K_r and above; old
    never = np.full((20, 2), -1, np.int32)
    never[4], never[11] = (5, 6), (7, -1)                                  # K_r = 5: every entry names no cluster
    hot = np.full((2000, 2), -1, np.int32)
    hot[:, 0] = 1
    hot[1000:, 1] = 0
    none = np.full((10, 2), -1, np.int32)
    none[2] = (0, 1)                                                       # K_r = 0
    tabs = [both, never, scattered(257, 600), scattered(300, 700), np.zeros((0, 2), np.int32), hot, none]
    names = ["both_slots_new", "never_seen", "K257", "K300", "no_frames", "contention", "no_clusters"]
    return tabs, offsets([len(t) for t in tabs]), offsets([4, 5, 257, 300, 3, 2, 0]), names


def speakers_tables(frame_counts, cluster_counts, seed=42):
    """Random speakers (entries up to K_r + 1) over given frame and cluster counts."""
    rng = np.random.default_rng(seed)
    return [np.where(rng.random((int(G), 2)) < 0.6, rng.integers(0, int(K) + 2, (int(G), 2)), -1).astype(np.int32)
            for G, K in zip(frame_counts, cluster_counts)], offsets(frame_counts), offsets(cluster_counts)


def labels_for(C, cent_off, seed=43):
    """C chunks spread over the recordings, labels in [-1, K_r + 3) -> (chunk_off, labels [C, 3])."""
    rng = np.random.default_rng(seed)
    R = len(cent_off) - 1
    counts = np.bincount(rng.integers(0, R, C), minlength=R) if C else np.zeros(R, np.int64)
    lab = [rng.integers(-1, int(k) + 3, (int(c), 3)) for c, k in zip(counts, np.diff(cent_off))]
    return offsets(counts), np.concatenate(lab).astype(np.int32).reshape(-1, 3)


def odd_centroids(K, d, seed=44):
    """fp32 and float64 rows that carry NaN, -0.0 and a denormal (compared through an integer view)."""
    rng = np.random.default_rng(seed)
    c32, c64 = rng.standard_normal((K, d)).astype(np.float32), rng.standard_normal((K, d))
    for c, tiny in ((c32, np.float32(1e-42)), (c64, 5e-320)):
        c[0::3, 1], c[1::3, d - 1], c[2::3, d // 2] = np.nan, -0.0, tiny
    return c32, c64


def renumber_expected(tabs, cent_off, chunk_off, labels):
    """DR.order_by_appearance per recording (entries at or above K_r are no cluster) -> (renum [K], labels rewritten, source row of every row)."""
    renum, lab2, src = np.zeros(int(cent_off[-1]), np.int32), labels.copy(), np.zeros(int(cent_off[-1]), np.int64)
    for r, sp in enumerate(tabs):
        b, e = int(cent_off[r]), int(cent_off[r + 1])
        K = e - b
        new = np.asarray(DR.order_by_appearance(np.where(sp < K, sp, -1), K), np.int64)
        renum[b:e] = new
        src[b + new] = np.arange(b, e)
        lab = lab2[int(chunk_off[r]):int(chunk_off[r + 1])]
        ok = (lab >= 0) & (lab < K)
        lab[ok] = new[lab[ok]]
    return renum, lab2, src


# ------------------------------------------------------------------------------------------------ the arbiters, applied recording by recording
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def reconstruct_reference(pack, maxsp):
    """DR.reconstruct per recording on the packed frame grid -> (count [G], speakers [G, 2], act per recording [G_r, max(K_r, 1)])."""
    G = int(pack["frame_off"][-1])
    count, speakers, acts = np.zeros(G, np.uint8), np.full((G, 2), -1, np.int32), []
    for r, n in enumerate(pack["n"]):
        a, b, g0, g1 = (int(pack[t][r + i]) for t in ("chunk_off", "frame_off") for i in (0, 1))
        rc, rs, ract, _ = DR.reconstruct(pack["cls"][a:b], pack["starts"][r], pack["labels"][a:b], max(pack["K_list"][r], 1), int(n), maxsp)
        count[g0:g1], speakers[g0:g1] = rc, rs
        acts.append(ract)
    return count, speakers, acts


def assign_reference(d, constrained):
    """-> (the pack of assign_edges, AR.assign per recording), computed once."""
    def make():
        case = assign_edges(d, ASSIGN_SEED[d])
        return case, [AR.assign(E_r, info_r, [], [], constrained=bool(constrained), cent=cent_r) for E_r, info_r, cent_r in case[5]]
    return cached(("assign", d, int(constrained)), make)


def check_assign(d, refs, chunk_off, labels, score, bound):
    """The existing grouped-assign test's three conditions -> (chunks with candidates, kept, max score error)."""
    total = kept = 0
    err = 0.0
    for r, ref in enumerate(refs):
        a, b = int(chunk_off[r]), int(chunk_off[r + 1])
        ok = ref["margin"] > (3 * d + 6) * 2.0 ** -52
        total, kept = total + int((ref["m"] > 0).sum()), kept + int(((ref["m"] > 0) & ok).sum())
        assert np.array_equal(labels[a:b][ok], ref["labels"][ok]), f"recording {r}"
        err = max(err, float(np.abs(score[a:b][ok] - ref["score"][ok]).max(initial=0.0)))
        assert np.array_equal(labels[a:b][ref["m"] == 0], np.full((int((ref["m"] == 0).sum()), 3), -1))
    assert kept >= 0.95 * total, (kept, total)
    assert err <= bound, err
    return total, kept, err
