"""CPU checks of the many-recordings diarization (diarize.pack_recordings and the numpy restatements of the grouped kernels): the packing
against chunk_starts and the zero-padded windows of every recording alone, the grouped restatements against the single-recording references
(tests/assign_ref.py, cluster.fold_small_clusters, tests/diarize_ref.py) applied recording by recording, bit for bit, and the new entry
points of the built library."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assign_ref as AR  # noqa: E402
import diarize_ref as DR  # noqa: E402
from conftest import sub  # noqa: E402
from test_diarize_gpu import random_cls  # noqa: E402

dz = sub("diarize")
seg = sub("segmentation")
cluster = sub("cluster")
LIB = sub("_lib")
CHUNK, RATE = 160000, 16000
LENGTHS = [0, 5 * RATE, CHUNK, CHUNK + 1, 23 * RATE + 333]
NEW_SYMBOLS = ["sdk_diarize_assign_grouped", "sdk_diarize_fold_grouped", "sdk_diarize_reconstruct_grouped", "sdk_diarize_first_seen",
               "sdk_diarize_renumber"]


# ------------------------------------------------------------------------------------------------ shared case builders (the GPU tests use them too)
def offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def assign_cases(d, seed):
    """Recordings from assign_ref.make_case over C_r in {0, 1, 7, 40} and K_r in {0, 1, 2, 5, 70} (K_r = 0: a K = 1 case whose centroids are
    withheld), plus one recording without chunks -> (E, info, cent64, chunk_off, cent_off, per-recording (E_r, info_r, cent_r))."""
    per = []
    for n, (Cn, K) in enumerate([(Cn, K) for Cn in (0, 1, 7, 40) for K in (0, 1, 2, 5, 70)]):
        E, info, tr, tl = AR.make_case(seed * 1000 + n, Cn, max(K, 1), d=d)
        cent = AR.centroids(E, info, tr, tl) if K else np.zeros((0, d))
        per.append((E, info, cent))
        if n == 7:
            per.append((np.zeros((0, d), np.float32), np.zeros((0, 3, 4), np.int32), np.zeros((0, d))))     # a recording without chunks
    E = np.concatenate([p[0] for p in per])
    info = np.concatenate([p[1] for p in per])
    cent = np.concatenate([p[2] for p in per])
    return E, info, cent, offsets([p[1].shape[0] for p in per]), offsets([p[2].shape[0] for p in per]), per


def fold_cases(seed, d=64):
    """Per recording: unit rows around K_r well-separated centres, canonical labels, sizes mixing clusters below and above the effective
    minimum; one recording without a large cluster, one with all clusters large -> list of (E float64 [N, d], labels, min_cluster_size)."""
    rng = np.random.default_rng(seed)
    out = []
    for sizes, mcs in [([9, 1, 7, 2, 1, 8], 5), ([2] * 15, 7), ([6, 7, 9], 4), ([30, 2, 3, 25, 1, 1, 2, 40, 3], 12), ([3], 2),
                       ([2] * 70 + [9, 8, 1, 1], 6)]:
        K = len(sizes)
        centres = rng.standard_normal((K, d))
        centres /= np.linalg.norm(centres, axis=1, keepdims=True)
        lab = np.concatenate([np.arange(K), rng.permutation(np.repeat(np.arange(K), np.asarray(sizes) - 1))])   # first appearances in label order: canonical
        E = centres[lab] + 0.3 * rng.standard_normal((len(lab), d)) / np.sqrt(d)
        E = (E / np.linalg.norm(E, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
        assert np.array_equal(cluster.canonical_labels(lab), lab)
        out.append((E, lab.astype(np.int32), mcs))
    return out


def fold_tables(cases):
    """-> (unit float64 centroids of the cut [Kc, d], sizes, cl_off, eff, cent_off, the reference's labels and second-best margins)."""
    cents, sizes, eff, kept, ref, margins = [], [], [], [], [], []
    for E, lab, mcs in cases:
        K = int(lab.max()) + 1
        sz = np.bincount(lab, minlength=K)
        m = min(int(mcs), max(1, round(0.1 * len(lab))))
        c = np.zeros((K, E.shape[1]))
        np.add.at(c, lab, E)
        c /= sz[:, None]
        c /= np.linalg.norm(c, axis=1, keepdims=True)
        cents.append(c)
        sizes.append(sz)
        eff.append(m)
        large, small = np.flatnonzero(sz >= m), np.flatnonzero(sz < m)
        kept.append(max(1, large.size))
        ref.append(cluster.fold_small_clusters(E, lab, mcs)[0])
        if large.size > 1 and small.size:
            cos = np.sort(c[small] @ c[large].T, axis=1)
            margins.append(float((cos[:, -1] - cos[:, -2]).min()))
    return np.concatenate(cents), np.concatenate(sizes), offsets([len(s) for s in sizes]), np.asarray(eff), offsets(kept), ref, margins


def reconstruct_case(step_s, K_list, seed):
    """R = 5 recordings (0 samples, 5 s, exactly 10 s, 23 s + 333 samples, 31 s) -> (pack tables, cls, labels local, K per recording)."""
    n = np.array([0, 5 * RATE, CHUNK, 23 * RATE + 333, 31 * RATE], np.int64)
    rng = np.random.default_rng(seed)
    starts = [seg.chunk_starts(int(m), step_s) if m else np.zeros(0, np.int64) for m in n]
    cls = random_cls(rng, sum(len(s) for s in starts))
    labels = np.concatenate([rng.integers(-1, max(K, 1), (len(s), 3)) if K else np.full((len(s), 3), -1) for s, K in zip(starts, K_list)]).astype(np.int32)
    return n, starts, cls, labels, offsets([len(s) for s in starts]), offsets([dz.global_frames(int(m)) for m in n]), offsets(K_list)


def speakers_case(seed):
    """speakers tables of three recordings in which some clusters never surface and some first appear in slot 1."""
    rng = np.random.default_rng(seed)
    K_list, G_list = [6, 0, 1, 75], [400, 50, 30, 900]
    tabs = []
    for K, G in zip(K_list, G_list):
        sp = np.full((G, 2), -1, np.int32)
        if K:
            seen = rng.permutation(K)[:max(1, K - 2)]                       # two clusters (when there are that many) never surface
            for g in range(5, G):
                if rng.random() < 0.7:
                    sp[g, 0] = seen[int(rng.integers(0, min(len(seen), 1 + g // 8)))]
                    if rng.random() < 0.4 and len(seen) > 1:
                        k = seen[int(rng.integers(0, min(len(seen), 2 + g // 6)))]
                        if k != sp[g, 0]:
                            sp[g, 1] = k
        tabs.append(sp)
    return tabs, offsets(G_list), offsets(K_list)


# ------------------------------------------------------------------------------------------------ packing
@pytest.mark.parametrize("step_s", [1.0, 2.5])
def test_packing_keeps_every_chunk_inside_its_own_recording(step_s):
    recs = [np.full(n, 1000 + 7 * i, np.int16) for i, n in enumerate(LENGTHS)]
    p = dz.pack_recordings(recs, step_s)
    assert p.samples.dtype == np.int16 and p.starts_packed.dtype == np.int32 and p.starts_local.dtype == np.int32
    assert p.n_samples.tolist() == LENGTHS
    assert p.chunk_off[0] == 0 and p.frame_off[0] == 0 and len(p.chunk_off) == len(p.frame_off) == len(recs) + 1
    assert np.array_equal(np.diff(p.frame_off), [dz.global_frames(n) for n in LENGTHS]) and p.frame_off[1] == 0
    assert p.chunk_off[-1] == len(p.starts_packed) == len(p.starts_local)
    for r, x in enumerate(recs):
        a, b = int(p.chunk_off[r]), int(p.chunk_off[r + 1])
        want = seg.chunk_starts(len(x), step_s) if len(x) else np.zeros(0, np.int64)
        assert np.array_equal(p.starts_local[a:b], want)
        o = int(p.rec_off[r])
        assert np.array_equal(p.samples[o:o + len(x)], x) and not p.samples[o + len(x):o + len(x) + CHUNK].any()     # the gap, the last one too
        assert o + len(x) + CHUNK <= len(p.samples)
        for c in range(a, b):
            s = int(p.starts_local[c])
            alone = np.pad(x[s:s + CHUNK], (0, max(0, s + CHUNK - len(x))))
            assert p.starts_packed[c] == o + s
            assert np.array_equal(p.samples[p.starts_packed[c]:p.starts_packed[c] + CHUNK], alone)
    assert len(p.samples) == sum(LENGTHS) + CHUNK * len(LENGTHS)
    empty = dz.pack_recordings([np.zeros(0, np.int16)], step_s)
    assert empty.chunk_off.tolist() == [0, 0] and empty.frame_off.tolist() == [0, 0] and len(empty.samples) == CHUNK


# ------------------------------------------------------------------------------------------------ host restatements
@pytest.mark.parametrize("constrained", [False, True])
def test_assign_grouped_host_equals_the_reference_per_recording(constrained):
    E, info, cent, chunk_off, cent_off, per = assign_cases(64, 3)
    labels, score = dz.assign_grouped_host(E, info, cent, chunk_off, cent_off, constrained)
    kept = total = 0
    for r, (E_r, info_r, cent_r) in enumerate(per):
        a, b = int(chunk_off[r]), int(chunk_off[r + 1])
        ref = AR.assign(E_r, info_r, [], [], constrained=constrained, cent=cent_r)
        ok = ref["margin"] > (3 * 64 + 6) * 2.0 ** -52                   # decisions the summation order cannot move
        total, kept = total + int((ref["m"] > 0).sum()), kept + int(((ref["m"] > 0) & ok).sum())
        assert np.array_equal(labels[a:b][ok], ref["labels"][ok])
        assert np.abs(score[a:b][ok] - ref["score"][ok]).max(initial=0.0) <= 1e-12
    assert kept >= 0.95 * total


def test_fold_grouped_host_equals_fold_small_clusters_per_recording():
    cases = fold_cases(5)
    cent, sizes, cl_off, eff, cent_off, ref, margins = fold_tables(cases)
    assert min(margins) > 1e-9
    remap = dz.fold_grouped_host(cent, sizes, cl_off, eff, cent_off)
    for r, (E, lab, _) in enumerate(cases):
        assert np.array_equal(remap[int(cl_off[r]) + lab] - cent_off[r], ref[r])
    assert (np.diff(cent_off) == [3, 1, 3, 3, 1, 2]).all()


@pytest.mark.parametrize("step_s,maxsp", [(1.0, None), (2.5, 1), (1.0, 0)])
def test_reconstruct_grouped_host_equals_the_reference_per_recording(step_s, maxsp):
    K_list = [3, 0, 1, 70, 3]
    n, starts, cls, labels, chunk_off, frame_off, cent_off = reconstruct_case(step_s, K_list, 11)
    count, speakers, acts = dz.reconstruct_grouped_host(cls, np.concatenate(starts), labels, chunk_off, frame_off, n, cent_off, maxsp)
    for r in range(len(n)):
        a, b, g0, g1 = int(chunk_off[r]), int(chunk_off[r + 1]), int(frame_off[r]), int(frame_off[r + 1])
        if a == b:
            assert g0 == g1
            continue
        rc, rs, ract, _ = DR.reconstruct(cls[a:b], starts[r], labels[a:b], max(K_list[r], 1), int(n[r]), maxsp)
        assert np.array_equal(count[g0:g1], rc) and np.array_equal(speakers[g0:g1], rs) and np.array_equal(acts[r], ract)


def test_first_seen_and_renumber_host_equal_order_by_appearance():
    tabs, frame_off, cent_off = speakers_case(2)
    first = dz.first_seen_host(np.concatenate(tabs), frame_off, cent_off)
    K = int(cent_off[-1])
    rng = np.random.default_rng(0)
    chunk_off = offsets([9, 4, 3, 20])
    labels = np.concatenate([rng.integers(-1, max(k, 1), (c, 3)) if k else np.full((c, 3), -1) for c, k in zip(np.diff(chunk_off), np.diff(cent_off))]).astype(np.int32)
    cent = rng.standard_normal((K, 8))
    renum, lab2, cent2 = dz.renumber_host(first, cent_off, chunk_off, labels, cent)
    slot1 = never = 0
    for r, sp in enumerate(tabs):
        b, e = int(cent_off[r]), int(cent_off[r + 1])
        new = np.asarray(DR.order_by_appearance(sp, e - b), np.int64)
        assert np.array_equal(renum[b:e], new)
        assert np.array_equal(new, dz.appearance_order(sp, e - b))
        lab = labels[int(chunk_off[r]):int(chunk_off[r + 1])]
        assert np.array_equal(lab2[int(chunk_off[r]):int(chunk_off[r + 1])], np.where(lab >= 0, new[np.maximum(lab, 0)] if e > b else -1, -1))
        if e > b:
            assert np.array_equal(cent2[b:e], cent[b:e][np.argsort(new)])
        never += int((first[b:e] == np.iinfo(np.int32).max).sum())
        slot1 += int((first[b:e][first[b:e] != np.iinfo(np.int32).max] % 2 == 1).sum())
    assert never >= 3 and slot1 >= 1, (never, slot1)


# ------------------------------------------------------------------------------------------------ the library's new entry points
def test_new_symbols_are_exported_and_declared():
    lib = C.CDLL(str(LIB.LIB_PATH))
    header = (LIB._HERE.parent / "include" / "sdk_hip.h").read_text()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported by libsdk_hip.so"
        assert name in LIB.SIGNATURES and f"int {name}(sdk_ctx* ctx" in header
    assert lib.sdk_abi_version() == LIB.ABI_VERSION == 4
