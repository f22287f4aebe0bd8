"""GPU checks of speaker-attributed transcripts (csrc/words.hip, words.py): sdk_words_attribute's rows, sdk_words_cooccur's table and
tallies and sdk_score_map's correct and map, bit for bit against the loop reference of tests/words_ref.py at every edge the rule names and
on seeded random packs; the library's refusals; then backend.diarize_transcript on the generated audio of tests/test_diarize_gpu.py.
Every comparison is integer equality."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_diarize_gpu as TG
import words_ref as WR
from conftest import sub

wd = sub("words")
ops_score = sub("ops_score")
segs = sub("segments")
LIB = sub("_lib")
pytestmark = pytest.mark.gpu

PACKS = WR.edge_packs()


def as_results(recs):
    return [SimpleNamespace(speakers=sp, n_speakers=K) for sp, K, _ in recs]


def as_seconds(recs):
    return [[(s0 / WR.RATE, s1 / WR.RATE) for s0, s1 in words] for _, _, words in recs]


def device_rows(engine, gap, recs):
    return wd.attribute(engine, as_results(recs), as_seconds(recs), gap * WR.HOP / WR.RATE)


@functools.lru_cache(maxsize=None)
def reference_rows(name):
    gap, recs = PACKS[name] if isinstance(name, str) else WR.random_pack(name)
    return [WR.attribute_ref(sp, K, words, gap) for sp, K, words in recs]


@pytest.mark.parametrize("name", sorted(PACKS))
def test_rows_bit_for_bit_on_every_edge(engine, name):
    gap, recs = PACKS[name]
    assert wd.gap_frames(gap * WR.HOP / WR.RATE) == gap
    got = device_rows(engine, gap, recs)
    for r, (lab, want) in enumerate(zip(got, reference_rows(name))):
        assert lab.rows.dtype == np.int32 and lab.rows.shape == want.shape and np.array_equal(lab.rows, want), (name, r, lab.rows.tolist(), want.tolist())


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_rows_bit_for_bit_on_random_packs_and_twice_the_same_bytes(engine, seed):
    gap, recs = WR.random_pack(seed)
    got, again = device_rows(engine, gap, recs), device_rows(engine, gap, recs)
    for r, (lab, want) in enumerate(zip(got, reference_rows(seed))):
        assert np.array_equal(lab.rows, want), (seed, r, np.argwhere(lab.rows != want)[:4].tolist())
        assert lab.rows.tobytes() == again[r].rows.tobytes()
        assert np.array_equal(lab.speaker, want[:, 0]) and np.array_equal(lab.distance, want[:, 6])


# (seed, K_r, S_r) and, where the word counts are fixed, W_r.  "straddle": sdk_words_cooccur's workgroups take 1024 words, so the first serves
# recording 1 and the head of recording 2, the second the tail of recording 2, then recordings 3 and 4; recording 0 has no word.
WDER_CASES = {"small": (31, (0, 1, 3, 5, 6), (4, 0, 6, 1, 3)), "small2": (32, (6, 5, 0, 3, 1), (0, 6, 2, 5, 4)), "wide": (33, (64, 3, 64, 1, 0), (3, 64, 64, 0, 1)),
              "straddle": (34, (3, 2, 5, 4, 3), (2, 3, 4, 5, 2), (0, 3, 1024 + 17, 301, 5))}


def wder_case(case):
    """The recordings (speakers, K, words) and reference labels of WDER_CASES[case]."""
    seed, K_r, S_r, *fixed = WDER_CASES[case]
    rng = np.random.default_rng(seed)
    recs = []
    for r, K in enumerate(K_r):
        G = int(rng.integers(200, 1500))
        recs.append((WR.random_speakers(rng, G, K), K, WR.random_words(rng, G, fixed[0][r] if fixed else 0 if r == 2 and case == "small" else int(rng.integers(50, 300)))))
    return recs, [WR.random_reference(rng, len(words), S) for (_, _, words), S in zip(recs, S_r)]


@pytest.mark.parametrize("case", sorted(WDER_CASES))
def test_wder_tables_bit_for_bit(engine, case):
    """co, the tallies, correct and the map of a pack against the loops; correct against the brute force where the table can be enumerated,
    against scipy's assignment where it cannot (64 a side)."""
    from scipy.optimize import linear_sum_assignment
    recs, refs = wder_case(case)
    if case == "straddle":
        assert [len(words) for _, _, words in recs] == [0, 3, 1041, 301, 5] and all(max(K, len(set(ref))) <= 8 for (_, K, _), ref in zip(recs, refs))
    gap = 10
    pack = wd.attribute_pack(engine, as_results(recs), as_seconds(recs), gap * WR.HOP / WR.RATE)
    got, again = wd.wder_pack(engine, pack, refs), wd.wder_pack(engine, pack, refs)
    rows = pack.rows.cpu().numpy()
    for r, ((sp, K, words), ref, res) in enumerate(zip(recs, refs, got)):
        hyp = WR.attribute_ref(sp, K, words, gap)[:, 0]
        assert np.array_equal(rows[int(pack.word_off[r]):int(pack.word_off[r + 1]), 0], hyp)
        exact = max(K, len(set(ref))) <= 8
        want = WR.wder_ref(hyp, ref, K, exact=exact)
        assert list(res.mapping) == want["names"] and res.co.shape == want["co"].shape and np.array_equal(res.co, want["co"]), (case, r)
        assert (res.scored, res.unassigned, res.words) == (want["scored"], want["unassigned"], len(words)), (case, r)
        if exact:
            assert res.correct == want["correct"] and res.wder == want["wder"], (case, r)
        elif res.co.size:
            i, j = linear_sum_assignment(want["co"], maximize=True)
            assert res.correct == int(want["co"][i, j].sum()), (case, r)
        m = list(res.mapping.values())
        used = [j for j in m if j >= 0]
        assert len(set(used)) == len(used) and sum(int(res.co[i, j]) for i, j in enumerate(m) if j >= 0) == res.correct
        host = wd.wder_host(hyp, ref, K)
        assert (host.correct, host.scored, host.unassigned) == (res.correct, res.scored, res.unassigned) and np.array_equal(host.co, res.co)
        assert again[r].mapping == res.mapping and again[r].correct == res.correct and again[r].co.tobytes() == res.co.tobytes()
    pooled = wd.pool(got)
    assert pooled.scored == sum(r.scored for r in got) and pooled.wder == wd.wder_value(pooled.scored, pooled.correct)
    print(f"wder {case}: {[round(r.wder, 4) for r in got]} pooled {pooled.wder:.4f} unassigned {pooled.unassigned}")


def test_refusals_are_exceptions_not_faults(engine):
    dev = engine.device
    up = lambda a, t=np.int32: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(t))).to(dev)  # noqa: E731
    sp, words, off2 = up(np.zeros((10, 2))), up([[0, 3000]]), up([0, 1])
    frame_off, cent_off = up([0, 10]), up([0, 1025])
    # the host layers refuse first ...
    with pytest.raises(ValueError, match="1025 hypothesis speakers"):
        wd.attribute(engine, [SimpleNamespace(speakers=np.zeros((10, 2), np.int32), n_speakers=1025)], [[(0.0, 0.2)]])
    with pytest.raises(ValueError, match="at most 1024"):
        ops_score.words_attribute(engine, words, off2, sp, frame_off, cent_off, 1025, 29)
    with pytest.raises(ValueError, match="must be a contiguous int32 device tensor"):
        ops_score.words_attribute(engine, words.cpu(), off2, sp, frame_off, cent_off, 1, 29)
    with pytest.raises(ValueError, match="word 0"):
        wd.attribute(engine, [SimpleNamespace(speakers=np.zeros((10, 2), np.int32), n_speakers=1)], [[(float("nan"), 0.2)]])
    # ... and the library refuses on its own, before any launch
    out = torch.full((1, 8), -7, dtype=torch.int32, device=dev)
    rc = engine.lib.sdk_words_attribute(engine.ctx, words.data_ptr(), off2.data_ptr(), sp.data_ptr(), frame_off.data_ptr(), cent_off.data_ptr(), 1, 1, 10, 1025, 29,
                                        out.data_ptr(), None)
    assert rc != 0 and b"at most 1024" in engine.lib.sdk_last_error()
    with pytest.raises(LIB.SdkError, match="at most 1024"):
        LIB.check(rc, "sdk_words_attribute")
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7).all()
    rows, ref, co_off = up(np.zeros((1, 8))), up([0]), up([0, 65], np.int64)
    for max_ref, max_hyp in ((65, 1), (1, 65)):
        with pytest.raises(LIB.SdkError, match="at most 64 each"):
            ops_score.words_cooccur(engine, rows, ref, off2, up([0, 1]), up([0, 1]), co_off, max_ref, max_hyp, 65)
    with pytest.raises(ValueError, match="65 reference and 1 hypothesis speakers; at most 64"):
        pack = wd.attribute_pack(engine, [SimpleNamespace(speakers=np.zeros((10, 2), np.int32), n_speakers=1)], [[(0.0, 0.1)] * 65])
        wd.wder_pack(engine, pack, [[f"r{i}" for i in range(65)]])
    # a K_r above the stated max_hyp is read as the counters' size, never past them: speaker 100 of "200" with max_hyp = 64 names nobody
    sp2 = up(np.full((10, 2), 100))
    got = ops_score.words_attribute(engine, words, off2, sp2, frame_off, up([0, 200]), 64, 29).cpu().numpy()
    assert got.tolist() == [[-1, 0, 0, 10, -1, 0, -1, 0]]


def test_diarize_transcript_end_to_end(engine, monkeypatch):
    """A few seconds of the generated scenario and an OpenAI-layout transcript written here: the relabelled document parses with
    segments.sentence_segments and its word speakers are attribute_host on the result's own speakers table."""
    for k in ("SDK_MODEL", "SDK_NO_TORCH", "SDK_PRECISION", "SDK_RESNET_WEIGHTS", "SDK_SEGMENTATION_WEIGHTS", "SDK_DIARIZE_MODEL"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SDK_DIARIZE_BATCH", "5")
    bk = sub("backend")
    be = bk.Backend()
    pcm, _, _ = TG.scenario()
    pcm = pcm[:12 * TG.RATE]
    rng = np.random.default_rng(3)
    starts = np.sort(rng.uniform(0.0, 11.5, 40)).round(2)
    transcript = {"task": "transcribe", "language": "english", "duration": 12.0, "text": " ".join(f"w{i}" for i in range(40)),
                  "words": [{"word": f"w{i}", "start": float(s), "end": float(round(s + rng.uniform(0.05, 0.6), 2))} for i, s in enumerate(starts)]}
    relabelled, rows, result = bk.diarize_transcript(be, pcm, transcript, step_s=1.0, threshold=0.5, min_cluster_size=2)
    assert result.speakers.shape == (WR.global_frames(len(pcm)), 2) and rows.shape == (40, 8) and rows.dtype == np.int32
    words = wd.transcript_words(transcript)
    want = wd.attribute_host(result.speakers, result.n_speakers, wd.prepare_words(words), wd.gap_frames(0.5))
    assert np.array_equal(rows, want)
    assert np.array_equal(rows, WR.attribute_ref(result.speakers, result.n_speakers, wd.prepare_words(words).tolist(), 29))
    label = lambda k: "UU" if k < 0 else f"S{k + 1}"  # noqa: E731
    assert [w[3] for w in wd.transcript_words(relabelled)] == [label(int(k)) for k in rows[:, 0]]
    sent = segs.sentence_segments(relabelled)
    assert sent and sent[0]["start"] == words[0][0] and sent[-1]["end"] == words[-1][1]
    assert [s["speaker"] for s in sent] == [label(s["speaker"]) for s in wd.attributed_sentences(transcript, rows)]
    per, pooled = bk.score_words(be, [result], [relabelled])              # scored against itself: no error but the words nobody got
    assert per[0].words == 40 and per[0].scored == int((rows[:, 0] >= 0).sum()) and per[0].wder == 0.0 and pooled.correct == per[0].scored
    print(f"e2e: K={result.n_speakers}, speakers {np.unique(rows[:, 0]).tolist()}, fallback words {int((rows[:, 6] > 0).sum())}, {len(sent)} sentences")
