"""CPU checks of the diarization pipeline's host side (diarize.py) against the loop-form rules of tests/diarize_ref.py, hand-made cases of the
stitching, the RTTM text, and the new entry points of the built library."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diarize_ref as DR  # noqa: E402
import resnet_ref as RR  # noqa: E402
from conftest import sub  # noqa: E402

dz = sub("diarize")
seg = sub("segmentation")
F = 589


def random_cls(rng, C, p_sil=0.3):
    """Class tables in runs (speech-like), every class present."""
    cls = np.zeros((C, F), np.uint8)
    for c in range(C):
        i = 0
        while i < F:
            n = int(rng.integers(1, 90))
            cls[c, i:i + n] = 0 if rng.random() < p_sil else rng.integers(1, 7)
            i += n
    return cls


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_decode_and_masks_match_the_rules(seed):
    rng = np.random.default_rng(seed)
    logp = rng.standard_normal((3, F, 7)).astype(np.float32)
    logp[0, :50, 2] = logp[0, :50, 5] = 9.0                              # ties: the lower class
    logp[1, :50] = 0.0
    got = dz.decode_host(logp)
    assert np.array_equal(got, DR.decode(logp)) and (got[0, :50] == 2).all() and (got[1, :50] == 0).all()
    cls = random_cls(rng, 6)
    cls[4] = 4                                                           # never alone: the full columns are used
    cls[5, 10:] = 0                                                      # 10 frames: two columns or fewer
    for T4 in (126, 26, 7):
        w, info = dz.masks_host(cls, T4)
        rw, rinfo = DR.masks(cls, T4)
        assert np.array_equal(w, rw) and np.array_equal(info, rinfo)
    w, info = dz.masks_host(cls, 126)
    assert info[4, 0].tolist() == [F, 0, 0, 1] and info[4, 2].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("step_s,n_s,K,maxsp", [(1.0, 23.0, 5, None), (0.5, 14.3, 1, None), (2.5, 31.7, 70, 1), (1.0, 7.0, 3, None), (1.0, 12.0, 4, 0)])
def test_reconstruct_matches_the_rules_and_aggregate_counts_mapping(step_s, n_s, K, maxsp):
    n = int(n_s * 16000) + 77
    st = seg.chunk_starts(n, step_s)
    rng = np.random.default_rng(int(n_s * 10) + K)
    cls = random_cls(rng, len(st))
    labels = rng.integers(-1, K, (len(st), 3)).astype(np.int32)
    count, speakers, act, nc = dz.reconstruct_host(cls, st, labels, K, n, maxsp)
    rcount, rspeakers, ract, rnc = DR.reconstruct(cls, st, labels, K, n, maxsp)
    assert np.array_equal(act, ract) and np.array_equal(nc, rnc)
    assert np.array_equal(count, rcount) and np.array_equal(speakers, rspeakers)
    # the same grid and the same contributing chunks as segmentation.aggregate_counts: G frames, and speech / overlap by its rule from nc
    G = dz.global_frames(n)
    assert count.shape == (G,) and G == max(0, (n - 495 + 269) // 270)
    counts = np.array([[len(DR.CLASSES[v]) for v in row] for row in cls])
    speech, overlap = seg.aggregate_counts(counts, st, n)
    sp = np.zeros(G)
    for c in range(len(st)):
        q = (135 - int(st[c])) // 270
        for i in range(F):
            if 0 <= i - q < G:
                sp[i - q] += counts[c, i] >= 1
    assert speech == seg.frames_to_ranges((nc > 0) & (2 * sp >= nc))
    assert (nc[:G - 3] > 0).all() and not count[nc == 0].any()          # only the recording's last frames lie past every chunk's 589 frames


def test_assignment_training_filter_order_and_turns_match_the_rules():
    rng = np.random.default_rng(5)
    C = 9
    cls = random_cls(rng, C)
    _, info = dz.masks_host(cls, 126)
    base = rng.standard_normal((3, 16))
    E = np.stack([base[r % 3] + 0.05 * rng.standard_normal(16) for r in range(3 * C)])
    E = (E / np.linalg.norm(E, axis=1, keepdims=True)).astype(np.float32)
    train = dz.training_rows(info, F)
    assert list(train) == DR.training(info, F) and 0 < len(train) < 3 * C
    tl = np.array([r % 3 for r in train], np.int32)
    labels, cent = dz.assign_rows(E, info, train, tl)
    rlabels, rcent, margins = DR.assign(E, info, list(train), list(tl))
    assert np.array_equal(labels, rlabels) and np.allclose(cent, rcent, atol=1e-6) and min(margins) > 0.1
    n = int(seg.chunk_starts(18 * 16000, 1.0)[-1]) + 160000
    st = seg.chunk_starts(n, 1.0)
    assert len(st) == C
    _, speakers, _, _ = dz.reconstruct_host(cls, st, labels, 3, n)
    new = dz.appearance_order(speakers, 3)
    assert list(new) == DR.order_by_appearance(speakers, 3)
    assert list(dz.appearance_order(np.array([[2, -1], [2, 0], [-1, -1]]), 4)) == [1, 2, 0, 3]
    assert dz.turns_from_frames(speakers, 3) == DR.turns(speakers, 3)
    # no training row: one cluster of the valid active rows; nothing valid: no cluster
    l1, c1 = dz.assign_rows(E, info, np.zeros(0, np.int64), np.zeros(0, np.int32))
    r1, rc1, _ = DR.assign(E, info, [], [])
    assert np.array_equal(l1, r1) and c1.shape == (1, 16) and np.allclose(c1, rc1, atol=1e-6) and set(np.unique(l1)) <= {-1, 0}
    l0, c0 = dz.assign_rows(E, np.zeros_like(info), np.zeros(0, np.int64), np.zeros(0, np.int32))
    assert (l0 == -1).all() and c0.shape == (0, 16)


def _two_chunk_case():
    """12 s, chunks at 0 and 2 s (the last start, 32 000, is not a multiple of 270).  Voice A speaks 1 - 4 s, voice B 5 - 8 s, both 8 - 9 s;
    chunk 0 calls them local 0 / 1, chunk 1 local 2 / 0 (permuted)."""
    n = 12 * 16000
    st = seg.chunk_starts(n, 2.0)
    assert st.tolist() == [0, 32000] and st[-1] % 270 != 0
    cls = np.zeros((2, F), np.uint8)
    local = [{"A": 0, "B": 1}, {"A": 2, "B": 0}]
    single = {0: 1, 1: 2, 2: 3}
    pair = {frozenset((0, 1)): 4, frozenset((0, 2)): 5, frozenset((1, 2)): 6}
    for c in range(2):
        for i in range(F):
            t = (int(st[c]) + 270 * i + 495) / 16000
            on = [v for v, (a, b) in (("A", (1, 4)), ("A", (8, 9)), ("B", (5, 9))) if a <= t < b]
            ids = {local[c][v] for v in on}
            cls[c, i] = 0 if not ids else single[next(iter(ids))] if len(ids) == 1 else pair[frozenset(ids)]
    labels = np.array([[0, 1, -1], [1, -1, 0]], np.int32)
    return n, st, cls, labels


def test_permuted_local_speakers_are_stitched_into_continuous_turns():
    n, st, cls, labels = _two_chunk_case()
    count, speakers, act, nc = dz.reconstruct_host(cls, st, labels, 2, n)
    assert np.array_equal(speakers, DR.reconstruct(cls, st, labels, 2, n)[1])
    tn = dz.turns_from_frames(speakers, 2)
    assert [k for _, _, k in tn] == [0, 1, 0]                            # A 1 - 4, B 5 - 9, A 8 - 9 (simultaneous with B)
    for (a, b, _), (wa, wb) in zip(tn, [(1, 4), (5, 9), (8, 9)]):
        assert abs(a - wa) < 0.03 and abs(b - wb) < 0.03
    assert count.max() == 2 and (count[int(8.2 * 16000 / 270):int(8.8 * 16000 / 270)] == 2).all()
    # max_speakers = 1: the overlap keeps the cluster seen by more chunks, or the lower one on a tie
    c1, s1, _, _ = dz.reconstruct_host(cls, st, labels, 2, n, 1)
    assert c1.max() == 1 and (s1[:, 1] == -1).all() and np.array_equal(s1, DR.reconstruct(cls, st, labels, 2, n, 1)[1])
    g = int(8.5 * 16000 / 270)
    assert act[g].tolist() == [2, 2] and speakers[g].tolist() == [0, 1] and s1[g].tolist() == [0, -1]      # the tie: the lower cluster
    # count = 1 and no labelled cluster active: no speaker
    c2, s2, _, _ = dz.reconstruct_host(cls, st, np.full((2, 3), -1, np.int32), 1, n)
    assert c2.max() == 2 and (s2 == -1).all() and dz.turns_from_frames(s2, 0) == []
    # the count is the mean over the chunks rounded half up, at most 2
    cls3 = cls.copy()
    cls3[1] = 0
    c3, _, _, nc3 = dz.reconstruct_host(cls3, st, labels, 2, n)
    both = nc3 == 2
    assert (c3[both] == ((np.array([len(DR.CLASSES[v]) for v in cls3[0]])[np.flatnonzero(both)] + 1) // 2)).all()


def test_silence_and_short_recordings():
    n = 7 * 16000
    st = seg.chunk_starts(n, 1.0)
    assert st.tolist() == [0]
    cls = np.zeros((1, F), np.uint8)
    count, speakers, _, nc = dz.reconstruct_host(cls, st, np.full((1, 3), -1, np.int32), 1, n)
    G = dz.global_frames(n)
    assert G == 413 and count.shape == (G,) and not count.any() and (speakers == -1).all() and (nc == 1).all()
    _, info = dz.masks_host(cls, 126)
    assert not info.any() and len(dz.training_rows(info, F)) == 0
    cls[0, 100:200] = 1
    count, speakers, _, _ = dz.reconstruct_host(cls, st, np.array([[0, -1, -1]], np.int32), 1, n)
    assert dz.turns_from_frames(speakers, 1) == [((270 * 100 + 360) / 16000, (270 * 199 + 630) / 16000, 0)]
    assert dz.global_frames(100) == 0


def test_rttm_text():
    tn = [(1.00125, 3.5, 0), (3.25, 4.0, 11)]
    text = dz.to_rttm(tn, "rec1")
    assert text == DR.rttm(tn, "rec1")
    assert text.splitlines()[0] == "SPEAKER rec1 1 1.001 2.499 <NA> <NA> SPEAKER_00 <NA> <NA>"
    assert text.splitlines()[1] == "SPEAKER rec1 1 3.250 0.750 <NA> <NA> SPEAKER_11 <NA> <NA>"
    assert dz.to_rttm([], "x") == ""


def test_last_map_restatement_reproduces_layer_boundary_embed():
    """diarize_ref.last_map + all-ones weights = resnet_ref.layer_boundary_embed (the restated layer loop is the same model)."""
    rn = sub("resnet")
    w = rn.synthetic_weights(3)
    feats = RR.round_bits(torch.from_numpy(np.random.default_rng(3).standard_normal((2, 41, 80)).astype(np.float32)) * 3, 8)
    for bits in (8, 11, None):
        last = DR.last_map(w, feats, bits)
        got = DR.weighted_embed(w, last, torch.ones(2, 1, last.shape[-1]))[:, 0]
        want = RR.layer_boundary_embed(w, feats, bits)
        assert float((got - want).abs().max()) <= 1e-9 * float(want.abs().max())


def test_new_symbols_exist_in_the_built_library():
    lib = sub("_lib").load_library()
    for name in ("sdk_powerset_decode", "sdk_diarize_masks", "sdk_diarize_reconstruct", "sdk_diarize_frames", "sdk_resnet_forward_masked",
                 "sdk_resnet_masked_workspace_bytes", "sdk_resnet_last_map_frames", "sdk_resnet_masked_pool", "sdk_resnet_pool"):
        assert hasattr(lib, name)
    rn = sub("resnet")
    _, d = rn.pack_weights(rn.synthetic_weights(0))
    import ctypes as C
    assert lib.sdk_resnet_last_map_frames(C.byref(d), 1001) == 126 and lib.sdk_resnet_last_map_frames(C.byref(d), 201) == 26
    assert lib.sdk_resnet_masked_workspace_bytes(C.byref(d), 2, 1001, 3) > lib.sdk_resnet_workspace_bytes(C.byref(d), 2, 1001)
    assert lib.sdk_resnet_masked_workspace_bytes(C.byref(d), 2, 1001, 1) == lib.sdk_resnet_workspace_bytes(C.byref(d), 2, 1001)
    assert lib.sdk_diarize_frames(7 * 16000) == 413 and lib.sdk_diarize_frames(100) == 0
