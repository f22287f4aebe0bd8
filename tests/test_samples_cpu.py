"""CPU checks of samples.py: runs_host and score_host against the loop reference of tests/samples_ref.py on every edge pack and on seeded
packs, cut_clips and select on hand-made tables, write_samples, and every ValueError.  No GPU."""
from __future__ import annotations

import json
import wave

import numpy as np
import pytest

import samples_ref as SR
from conftest import sub

sm = sub("samples")
PACKS = SR.edge_packs()


@pytest.mark.parametrize("name", sorted(PACKS))
def test_runs_host_on_every_edge(name):
    gap, min_fr, recs = PACKS[name]
    for r, (sp, K) in enumerate(recs):
        got, want = sm.runs_host(sp, K, gap, min_fr), SR.runs_ref(sp, K, gap, min_fr)
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (name, r, got.tolist(), want.tolist())


def test_the_edge_packs_hold_what_they_claim():
    rows = {name: [SR.runs_ref(sp, K, gap, mf) for sp, K in recs] for name, (gap, mf, recs) in PACKS.items()}
    assert [len(x) for x in rows["silent_overlapped_solo"]] == [0, 0, 1] and rows["silent_overlapped_solo"][2].tolist() == [[1, 0, 100, 100]]
    assert rows["speakers_0_1_1024"][0].shape == (0, 4) and rows["speakers_0_1_1024"][1].tolist() == [[0, 3, 20, 17]]
    assert rows["speakers_0_1_1024"][2].tolist() == [[1023, 0, 4, 4], [1022, 6, 9, 3]]
    assert rows["neighbours"][0].tolist() == [[0, 30, 40, 10]] and rows["neighbours"][1].tolist() == [[0, 0, 7, 7], [1, 45, 50, 5]]
    assert rows["gap_exact"][0].tolist() == [[0, 2, 15, 8]] and rows["gap_exact"][1].tolist() == [[0, 2, 6, 4], [0, 12, 15, 3]]
    assert rows["gap_exact"][2].tolist() == [[0, 0, 7, 2], [0, 13, 20, 2]]
    assert rows["gap_zero"][0].tolist() == [[0, 2, 9, 7], [0, 10, 12, 2]] and rows["gap_zero"][2].tolist() == [[0, 1, 2, 1], [0, 3, 4, 1]]
    assert rows["nobody_entries"][0].tolist() == [[0, 0, 4, 3], [1, 6, 9, 3]]      # one silent frame (7, -3) is bridged at gap 1
    assert rows["forms"][0].tolist() == [[1, 0, 3, 3], [0, 3, 6, 3]] and rows["forms"][1].tolist() == [[0, 0, 1, 1], [1, 2, 3, 1]]
    assert rows["min_frames"][0].tolist() == [[0, 0, 5, 5], [0, 8, 16, 6]] and rows["min_frames"][1].tolist() == [[1, 10, 14, 4]] and len(rows["min_frames"][2]) == 0
    assert rows["single_frames"][0].tolist() == [[0, 0, 1, 1], [1, 2, 3, 1], [0, 5, 6, 1], [2, 8, 9, 1]]
    long_run = rows["long_run"][1]
    assert len(long_run) == 1 and long_run[0, 2] - long_run[0, 1] > 3 * SR.SPAN and long_run[0, 3] < long_run[0, 2] - long_run[0, 1]


@pytest.mark.parametrize("seed", [21, 22, 23])
def test_runs_host_on_random_packs(seed):
    gap, min_fr, recs = SR.random_pack(seed)
    n = 0
    for r, (sp, K) in enumerate(recs):
        got, want = sm.runs_host(sp, K, gap, min_fr), SR.runs_ref(sp, K, gap, min_fr)
        assert np.array_equal(got, want), (seed, r)
        n += len(want)
    assert n > 0


@pytest.mark.parametrize("d", sorted(SR.SCORE_CASES))
def test_score_host_against_the_loops(d):
    E, clip_off, clip_spk, spk_off = SR.score_case(*SR.SCORE_CASES[d])
    want = SR.score_ref(E, clip_off, clip_spk, spk_off)
    mean, out_f, out_i = sm.score_host(E, clip_off, clip_spk, spk_off)
    assert np.abs(mean - want["mean"]).max() <= 1e-12 and np.abs(out_f[:, 0] - want["own"]).max() <= 1e-12 and np.abs(out_f[:, 1] - want["rival"]).max() <= 1e-12
    assert np.array_equal(out_i[:, 0], want["rival_speaker"]) and np.array_equal(out_i[:, 1], want["windows"]) and np.array_equal(out_i[:, 2], want["alone"])
    assert want["alone"].sum() >= 2 and (want["windows"] == 0).sum() == 1 and (want["rival_speaker"] == -1).sum() >= 4
    print(f"samples_score d={d}: least rest_ratio {want['rest_ratio'][want['alone'] == 0].min():.3e} (0.1 asked), least rival_gap {want['rival_gap'].min():.3e} "
          f"(1e-9 asked); alone {int(want['alone'].sum())}, empty {int((want['windows'] == 0).sum())}, rival-less {int((want['rival_speaker'] == -1).sum())}")
    assert (want["rest_ratio"][want["alone"] == 0] >= 0.1).all() and (want["rival_gap"] > 1e-9).all()
    if d > 256:                                                                # the GPU test's condition at a partly (and a fully) live second column
        assert SR.second_column_weight(f"samples_score d={d}", E, clip_off, clip_spk, spk_off, want) > 100


def test_min_frames_and_gap():
    assert sm.min_frames_of(0.5) == 30 and sm.min_frames_of(0.0) == 1 and sm.min_frames_of(270 / 16000) == 1 and sm.min_frames_of(271 / 16000) == 2
    assert sm.min_frames_of(0.5) == SR.min_frames(0.5) and sm.gap_frames(1.0) == 59


def test_cut_clips_remainder_rule_and_candidates():
    rows = np.asarray([[0, 0, 100, 77], [1, 200, 230, 30], [0, 300, 340, 40]], np.int32)
    n = 270 * 340 + 300
    whole = sm.cut_clips(rows, n)
    assert whole.tolist() == [[0, 360, 27360, 77], [1, 54360, 62460, 30], [0, 81360, n, 40]]             # the last run is cut at the recording's end
    cut = sm.cut_clips(rows, n, max_clip_s=0.5)                                                       # 8 000 samples: 27 000 -> 4 clips, 8 100 -> 2, 10 740 -> 2
    first = cut[cut[:, 1] < 30000]
    assert first[:, 1].tolist() == [360, 360 + 6750, 360 + 13500, 360 + 20250] and first[:, 2].tolist() == [360 + 6750, 360 + 13500, 360 + 20250, 27360]
    assert first[:, 3].tolist() == [20, 19, 19, 19]                                                   # 77 = 4 * 19 + 1: the remainder to the first clip
    assert cut[4:6].tolist() == [[1, 54360, 58410, 15], [1, 58410, 62460, 15]] and cut[6:, 3].tolist() == [20, 20] and len(cut) == 8
    assert (cut[1:, 1] >= cut[:-1, 1]).all() and (np.diff(cut[:, 1:3], axis=1) <= 8000).all()
    odd = sm.cut_clips(np.asarray([[2, 1, 4, 2]]), 10 ** 6, max_clip_s=300 / 16000)                     # L = 810 into 3 clips of 270; solo 2 -> 1, 1, 0
    assert odd.tolist() == [[2, 630, 900, 1], [2, 900, 1170, 1], [2, 1170, 1440, 0]]
    top = sm.cut_clips(rows, n, max_clip_s=0.5, max_candidates=2)                                     # per speaker: solo descending, then start ascending
    assert top.tolist() == [[0, 360, 7110, 20], [1, 54360, 58410, 15], [1, 58410, 62460, 15], [0, 81360, 81360 + 5370, 20]]
    assert sm.cut_clips(rows, n, max_candidates=0).shape == (0, 4) and sm.cut_clips(np.zeros((0, 4)), 5).shape == (0, 4)


def test_select_order_caps_and_ties():
    #                 speaker start  end    solo
    clips = np.asarray([[0, 0, 16000, 50], [0, 20000, 36000, 50], [0, 40000, 48000, 20], [0, 50000, 66000, 60], [1, 70000, 86000, 40],
                        [1, 90000, 98000, 30], [0, 100000, 116000, 50], [2, 120000, 130000, 30]])
    own = np.asarray([0.9, 0.9, 0.95, 0.2, 0.0, 0.5, 0.9, 0.1])
    rival = np.asarray([0.1, 0.1, 0.3, 0.4, 0.0, 0.6, 0.1, 0.3])
    alone = np.asarray([0, 0, 0, 0, 1, 0, 0, 0])
    got = sm.select(clips, own, rival, alone)
    assert got == {0: [2, 0, 1, 6], 1: [4]}                                  # margin < 0 is out (3, 5, 7); ties in own and solo go by start; alone is eligible
    assert sm.select(clips, own, rival, alone, min_margin=-0.25) == {0: [2, 0, 1, 6, 3], 1: [5, 4], 2: [7]}       # alone clips last
    assert sm.select(clips, own, rival, alone, max_clips=2) == {0: [2, 0], 1: [4]} and sm.select(clips, own, rival, alone, max_clips=0) == {}
    assert sm.select(clips, own, rival, alone, max_total_s=1.5) == {0: [2, 0], 1: [4]}                # 0.5 + 1.0 s; the next clip would carry it past
    assert sm.select(clips, own, rival, alone, max_total_s=1.4999) == {0: [2], 1: [4]}                # taking stops: the shorter clip 6 behind is not tried
    assert sm.select(clips, own, rival, alone, max_total_s=0.4) == {}
    assert sm.select(clips, own, rival, alone, min_margin=0.8) == {0: [0, 1, 6], 1: [4]}
    assert sm.select(np.zeros((0, 4)), [], [], []) == {}
    picked = sm.select(clips, own, rival, alone)
    out_f, out_i = np.stack([own, rival], 1), np.stack([np.full(8, -1), np.ones(8), alone], 1)
    res = sm.as_samples(3, clips, picked, out_f, out_i)
    assert [s.start_s for s in res[0]] == [2.5, 0.0, 1.25, 6.25] and res[1][0].alone is True and res[0][0].recording == 3 and res[0][0].speaker == 0
    assert res[0][0].solo_s == 20 * 270 / 16000 and res[0][0].embedding is None and res[0][1].end_s == 1.0


def test_write_samples(tmp_path):
    bk = sub("backend")
    audio = (np.arange(40000) % 2000 - 1000).astype(np.int16)
    samples = {1: [sm.SpeakerSample(0, 1, 0.5, 1.25, 0.7, 0.9, 0.2, 0, False, np.ones(4, np.float32)), sm.SpeakerSample(0, 1, 2.0, 2.1, 0.1, 0.8, 0.3, 0, False)],
               0: [sm.SpeakerSample(0, 0, 0.0, 0.6, 0.6, 0.0, 0.0, -1, True)]}
    paths = bk.write_samples(tmp_path / "out", samples, audio)
    assert [str(p.relative_to(tmp_path / "out")) for p in paths] == ["S1/sample-001.wav", "S2/sample-001.wav", "S2/sample-002.wav"]
    with wave.open(str(paths[1]), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 16000, 12000)
        assert np.array_equal(np.frombuffer(w.readframes(12000), "<i2"), audio[8000:20000])
    meta = json.loads(paths[1].with_suffix(".json").read_text())
    assert meta == {"recording": 0, "speaker": 1, "start_s": 0.5, "end_s": 1.25, "solo_s": 0.7, "own": 0.9, "rival": 0.2, "rival_speaker": 0, "alone": False}
    with pytest.raises(ValueError, match="outside the recording"):
        bk.write_samples(tmp_path / "bad", {0: [sm.SpeakerSample(0, 0, 2.0, 3.0, 1.0, 0.0, 0.0, -1, True)]}, audio)


def test_value_errors():
    sp = np.zeros((4, 2), np.int32)
    with pytest.raises(ValueError, match="1025 hypothesis speakers"):
        sm.runs_host(sp, 1025, 3, 1)
    for gap, mf in ((-1, 1), (3, 0)):
        with pytest.raises(ValueError, match="runs_host: gap="):
            sm.runs_host(sp, 1, gap, mf)
    for bad in (float("nan"), -0.1, float("inf"), 1e9):
        with pytest.raises(ValueError, match="min_s="):
            sm.min_frames_of(bad)
        with pytest.raises(ValueError, match="max_gap_s="):
            sm.gap_frames(bad)
        with pytest.raises(ValueError, match="max_clip_s="):
            sm.cut_clips(np.zeros((0, 4)), 10, max_clip_s=bad)
        with pytest.raises(ValueError, match="max_total_s="):
            sm.select(np.zeros((0, 4)), [], [], [], max_total_s=bad)
    with pytest.raises(ValueError, match="at least one sample"):
        sm.cut_clips(np.zeros((0, 4)), 10, max_clip_s=0.0)
    with pytest.raises(ValueError, match="max_candidates=-1"):
        sm.cut_clips(np.zeros((0, 4)), 10, max_candidates=-1)
    with pytest.raises(ValueError, match="outside the recording"):
        sm.cut_clips(np.asarray([[0, 10, 20, 5]]), 3000)
    with pytest.raises(ValueError, match="max_clips=-2"):
        sm.select(np.zeros((0, 4)), [], [], [], max_clips=-2)
    with pytest.raises(ValueError, match="min_margin"):
        sm.select(np.zeros((0, 4)), [], [], [], min_margin=float("nan"))
    with pytest.raises(ValueError, match="1 own, 2 rival"):
        sm.select(np.zeros((2, 4)), [0.0], [0.0, 0.0], [0, 0])
    E = np.zeros((5, 64), np.float32)
    with pytest.raises(ValueError, match="ascending offsets"):
        sm.score_host(E, [0, 3, 2], [0, 0], [0, 1])
    with pytest.raises(ValueError, match="ascending offsets"):
        sm.score_host(E, [0, 6], [0], [0, 1])
    with pytest.raises(ValueError, match="prefix sums from 0"):
        sm.score_host(E, [0, 2], [0], [1, 2])
    with pytest.raises(ValueError, match=r"clip_spk must lie in \[0, 1\)"):
        sm.score_host(E, [0, 2], [1], [0, 1])
    bk = sub("backend")
    with pytest.raises(ValueError, match="2 recordings for 1 results"):
        bk.speaker_samples(None, [object()], [np.zeros(5, np.int16)] * 2)
    assert bk.speaker_samples(None, [], []) == []
