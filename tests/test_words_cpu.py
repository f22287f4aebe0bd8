"""CPU checks of words.py: attribute_host and wder_host against the loop reference of tests/words_ref.py on every edge pack and on seeded
random packs, the value errors, the properties of the word-level error rate, and the transcript side (Speechmatics golden, AssemblyAI and
OpenAI documents written here).  Every comparison is integer equality."""
from __future__ import annotations

import copy
import json

import numpy as np
import pytest

import words_ref as WR
from conftest import GOLDEN, sub

wd = sub("words")
segs = sub("segments")
score = sub("score")

PACKS = WR.edge_packs()


@pytest.mark.parametrize("name", sorted(PACKS))
def test_attribute_host_equals_the_loops_on_every_edge(name):
    gap, recs = PACKS[name]
    for r, (sp, K, words) in enumerate(recs):
        got = wd.attribute_host(sp, K, np.asarray(words, np.int64).reshape(-1, 2), gap)
        want = WR.attribute_ref(sp, K, words, gap)
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (name, r, got.tolist(), want.tolist())


def test_the_edges_are_the_ones_the_rule_names():
    """The reference's rows at the edges, written out: the packs hold the cases they claim to."""
    row = lambda name, r, i: WR.attribute_ref(*PACKS[name][1][r], PACKS[name][0])[i].tolist()  # noqa: E731
    assert row("no_frames", 0, 0) == [-1, 0, 0, 0, -1, 0, -1, 0]
    assert row("points", 0, 0) == [1, 1, 1, 1, -1, 0, 0, 0] and row("points", 0, 2) == [3, 1, 1, 1, -1, 0, 0, 19]
    assert row("points", 0, 5)[7] == 5 and row("points", 0, 6)[7] == 6                 # between two centres: the nearer; half way: the later
    assert row("ties", 0, 0) == [1, 2, 1, 3, 0, 2, 0, 0] and row("ties", 1, 0) == [1, 2, 0, 2, 2, 2, 0, 0]
    assert row("ties", 2, 0) == [3, 3, 3, 3, -1, 0, 0, 0] and row("ties", 3, 0) == [1, 2, 2, 3, 0, 1, 0, 0]
    assert [row("gap_edge", 0, i)[6] for i in range(4)] == [29, -1, 29, -1] and [row("gap_edge", 0, i)[0] for i in range(4)] == [0, -1, 0, -1]
    assert [row("gap_zero", 0, i)[0] for i in range(3)] == [-1, -1, 0]
    assert row("gap_sides", 0, 0) == [1, 0, 0, 1, -1, 0, 5, 55] and row("gap_sides", 0, 1)[:1] + row("gap_sides", 0, 1)[6:7] == [1, 4]
    assert row("neighbours", 1, 0) == [1, 0, 0, 1, -1, 0, 20, 0] and row("neighbours", 1, 1) == [1, 0, 0, 1, -1, 0, 19, 39]
    assert row("neighbours", 4, 0)[0] == -1 and row("neighbours", 4, 1)[0] == -1
    assert row("gap_long", 0, 0) == [0, 0, 0, 1, -1, 0, 90, 60] and row("gap_long", 0, 1)[0] == -1 and row("gap_long", 0, 2)[6] == 100
    assert row("gap_long", 0, 4) == [1, 0, 0, 1, -1, 0, 59, 240] and row("gap_long", 0, 5) == [0, 0, 0, 1, -1, 0, 74, 224]
    for K in (1, 64, 65, 1024):
        assert row(f"speakers_{K}", 0, 0)[0] == K - 1 and row(f"speakers_{K}", 0, 3)[0] == (K - 1 if K == 1 else K - 2)
    spans = WR.attribute_ref(*PACKS["spans"][1][0], 29)[:, 3].tolist()
    assert spans[:9] == [1, 2, 18, 63, 64, 65, 128, 129, 5000] and spans[9:] == [5100, 5200]


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_attribute_host_equals_the_loops_on_random_packs(seed):
    gap, recs = WR.random_pack(seed)
    kinds = np.zeros(3, np.int64)
    for r, (sp, K, words) in enumerate(recs):
        got = wd.attribute_host(sp, K, np.asarray(words, np.int64).reshape(-1, 2), gap)
        want = WR.attribute_ref(sp, K, words, gap)
        assert np.array_equal(got, want), (seed, r, np.argwhere(got != want)[:4].tolist())
        kinds += [(want[:, 6] == 0).sum(), (want[:, 6] > 0).sum(), (want[:, 0] < 0).sum()]
    assert (kinds > 0).all(), kinds                                # voted, fallback and unassigned words all occur


def test_prepare_words_and_value_errors():
    assert wd.prepare_words([(0.0, 1.0), (0.00003, 2.5, "x")]).tolist() == [[0, 16000], [0, 40000]]
    assert wd.prepare_words([(0.00004, 0.00004)]).tolist() == [[1, 1]] and wd.prepare_words([]).shape == (0, 2)
    assert wd.gap_frames(0.5) == 29 and wd.gap_frames(0.0) == 0 and WR.gap_frames(0.5) == 29
    for bad in [(float("nan"), 1.0), (-0.5, 1.0), (1.0, float("inf")), (0.0, 2.0 ** 31 / 16000)]:
        with pytest.raises(ValueError, match="word 1"):
            wd.prepare_words([(0.0, 1.0), bad])
    with pytest.raises(ValueError, match="max_gap_s"):
        wd.gap_frames(float("nan"))
    sp = np.zeros((4, 2), np.int32)
    assert wd.attribute_host(sp, 1024, np.asarray([[0, 2000]]), 29)[0, 0] == 0
    with pytest.raises(ValueError, match="1025 hypothesis speakers; at most 1024"):
        wd.attribute_host(sp, 1025, np.asarray([[0, 2000]]), 29)
    ref65 = [f"r{i}" for i in range(65)]
    with pytest.raises(ValueError, match="65 reference and 1 hypothesis speakers; at most 64"):
        wd.wder_host(np.zeros(65, np.int64), ref65)
    with pytest.raises(ValueError, match="at most 64"):
        wd.wder_host(np.arange(65), ["a"] * 65)
    with pytest.raises(ValueError, match="reference labels"):
        wd.wder_host(np.zeros(3, np.int64), ["a"])


@pytest.mark.parametrize("seed", [21, 22, 23])
def test_wder_host_equals_the_brute_force(seed):
    rng = np.random.default_rng(seed)
    for S, K, W in [(0, 3, 10), (3, 0, 10), (1, 1, 5), (4, 6, 200), (6, 4, 200), (5, 5, 60), (2, 3, 0)]:
        ref = WR.random_reference(rng, W, S)
        hyp = rng.integers(-1, max(K, 1), W) if K else np.full(W, -1)
        got, want = wd.wder_host(hyp, ref, K), WR.wder_ref(hyp, ref, K)
        assert list(got.mapping) == want["names"] and np.array_equal(got.co, want["co"]) and got.co.shape == want["co"].shape
        assert (got.scored, got.unassigned, got.words, got.correct) == (want["scored"], want["unassigned"], W, want["correct"])
        assert got.wder == want["wder"]
        m = [j for j in got.mapping.values() if j >= 0]
        assert len(set(m)) == len(m) and sum(int(got.co[i, j]) for i, j in enumerate(got.mapping.values()) if j >= 0) == got.correct


def test_wder_properties():
    rng = np.random.default_rng(5)
    names = ["ann", "bob", "cy", "di"]
    ref = [names[i] for i in rng.integers(0, 4, 300)]
    same = np.asarray([names.index(n) for n in ref])
    assert wd.wder_host(same, ref).wder == 0.0 and wd.wder_host(same, ref).correct == 300
    hyp = np.where(rng.random(300) < 0.2, rng.integers(0, 4, 300), same)
    base = wd.wder_host(hyp, ref, 4)
    assert 0.0 < base.wder < 0.3
    for _ in range(5):                                              # any renaming of the hypothesis speakers
        perm = rng.permutation(6)
        again = wd.wder_host(perm[hyp], ref, 6)
        assert (again.correct, again.wder, again.scored) == (base.correct, base.wder, base.scored)
        assert {n: int(perm[j]) for n, j in base.mapping.items()} == again.mapping or again.correct == base.correct
    gone = same.copy()
    gone[:50] = -1
    res = wd.wder_host(gone, ref, 4)
    assert res.unassigned == 50 and res.correct == 250 and res.wder == 1.0 - 250 / 300       # unassigned words are errors
    skip = list(ref)
    skip[:10] = [None] * 5 + ["UU"] * 5
    res = wd.wder_host(same, skip)
    assert res.scored == 290 and res.words == 300 and res.wder == 0.0
    assert wd.wder_host(np.zeros(0, np.int64), []).wder == 0.0
    pooled = wd.pool([base, res])
    assert pooled.scored == base.scored + 290 and pooled.wder == 1.0 - (base.correct + 290) / (base.scored + 290) and pooled.co is None


# ------------------------------------------------------------------------------------------------ the transcript side
def test_relabelling_the_golden_with_its_own_speakers_changes_nothing_downstream():
    data = json.loads((GOLDEN / "test_001-two-speakers.wav.speechmatics.json").read_text())
    before = copy.deepcopy(data)
    words = wd.transcript_words(data)
    names = segs.get_available_speakers(data)
    assert len(names) >= 2 and len(words) == sum(1 for it in data["results"] if it.get("type") == "word")
    assert all(w[3] in names for w in words) and [w[3] for w in words] == [w[0] for w in segs._sm_words(data)]
    out = wd.relabel_transcript(data, [names.index(w[3]) for w in words], names=names)
    assert data == before and out is not data                       # a deep copy
    assert segs.detect_transcript_format(out) == "speechmatics"
    for name in names:
        assert segs.extract_segments_as_tuples(out, name) == segs.extract_segments_as_tuples(data, name)
        assert segs.extract_segments_from_transcript(out, name) == segs.extract_segments_from_transcript(data, name)
    assert segs.sentence_segments(out) == segs.sentence_segments(data)
    for item in out["results"]:
        if item.get("type") == "word":
            assert item["speaker"] == item["alternatives"][0]["speaker"]
    # the other way round: every word to speaker 1 of 2, unnamed; punctuation follows the word before it
    flip = wd.relabel_transcript(data, np.ones(len(words), np.int64))
    assert segs.get_available_speakers(flip) == ["S2"]
    last = None
    for item in flip["results"]:
        if item.get("type") == "word":
            last = item["speaker"]
        elif item.get("type") == "punctuation" and last is not None:
            assert item["speaker"] == last
    assert wd.relabel_transcript(data, np.full(len(words), -1))["results"][0]["speaker"] == "UU"
    with pytest.raises(ValueError, match="speakers for the transcript"):
        wd.relabel_transcript(data, [0])
    # sentences from rows: every word voted for its own speaker over its whole span
    rows = np.zeros((len(words), 8), np.int32)
    rows[:, 0], rows[:, 1], rows[:, 3] = [names.index(w[3]) for w in words], 4, 4
    rows[0, 1] = 1
    sent = wd.attributed_sentences(data, rows)
    want = segs.sentence_segments(data)
    assert [(s["start"], s["end"]) for s in sent] == [(s["start"], s["end"]) for s in want]
    assert [names[s["speaker"]] for s in sent] == [s["speaker"] for s in want]
    assert sum(s["words"] for s in sent) == len(words) and sent[0]["min_votes_share"] == 0.25 and sent[1]["min_votes_share"] == 1.0
    assert sent[0]["text"].startswith(words[0][2])


AAI = {"id": "x", "utterances": [
    {"speaker": "A", "start": 0, "end": 1500, "text": "hello there you", "words": [
        {"text": "hello", "start": 0, "end": 400, "speaker": "A"}, {"text": "there", "start": 500, "end": 900, "speaker": "A"},
        {"text": "you", "start": 1000, "end": 1500}]},
    {"speaker": "B", "start": 2000, "end": 3000, "text": "fine thanks"}],
    "words": [{"text": "hello", "start": 0, "end": 400, "speaker": "A"}, {"text": "there", "start": 500, "end": 900, "speaker": "A"},
              {"text": "you", "start": 1000, "end": 1500, "speaker": "A"}, {"text": "fine", "start": 2000, "end": 2400, "speaker": "B"},
              {"text": "thanks", "start": 2500, "end": 3000, "speaker": "B"}]}
OPENAI = {"task": "transcribe", "language": "english", "duration": 3.2, "text": "Hello there. Fine thanks",
          "words": [{"word": "Hello", "start": 0.0, "end": 0.4}, {"word": "there", "start": 0.5, "end": 0.9}, {"word": " Fine", "start": 2.0, "end": 2.4},
                    {"word": "thanks", "start": 2.5, "end": 3.0}]}


def test_assemblyai_document():
    words = wd.transcript_words(AAI)
    assert words == [(0.0, 0.4, "hello", "A"), (0.5, 0.9, "there", "A"), (1.0, 1.5, "you", "A"), (2.0, 2.4, "fine", "B"), (2.5, 3.0, "thanks", "B")]
    before = copy.deepcopy(AAI)
    out = wd.relabel_transcript(AAI, [0, 0, 1, 1, 0])
    assert AAI == before and segs.detect_transcript_format(out) == "assemblyai"
    assert [(u["speaker"], u["start"], u["end"], u["text"]) for u in out["utterances"]] == [("S1", 0, 900, "hello there"), ("S2", 1000, 2400, "you fine"),
                                                                                             ("S1", 2500, 3000, "thanks")]
    assert [w["speaker"] for w in out["words"]] == ["S1", "S1", "S2", "S2", "S1"] and out["id"] == "x"
    assert segs.sentence_segments(out) == [{"speaker": "S1", "start": 0.0, "end": 0.9}, {"speaker": "S2", "start": 1.0, "end": 2.4},
                                           {"speaker": "S1", "start": 2.5, "end": 3.0}]
    assert [w[3] for w in wd.transcript_words(out)] == ["S1", "S1", "S2", "S2", "S1"]
    named = wd.relabel_transcript(AAI, [0, 0, 0, -1, 1], names=["ann", "bob"])
    assert [u["speaker"] for u in named["utterances"]] == ["ann", "UU", "bob"]


def test_openai_document():
    words = wd.transcript_words(OPENAI)
    assert words == [(0.0, 0.4, "Hello", None), (0.5, 0.9, "there", None), (2.0, 2.4, "Fine", None), (2.5, 3.0, "thanks", None)]
    out = wd.relabel_transcript(OPENAI, [0, 0, 1, 1])
    assert segs.detect_transcript_format(out) == "speechmatics" and segs.get_available_speakers(out) == ["S1", "S2"]
    assert segs.sentence_segments(out) == [{"speaker": "S1", "start": 0.0, "end": 0.9}, {"speaker": "S2", "start": 2.0, "end": 3.0}]
    assert segs.extract_segments_as_tuples(out, "S2") == [(2.0, 3.0)]
    assert wd.transcript_words(out) == [(0.0, 0.4, "Hello", "S1"), (0.5, 0.9, "there", "S1"), (2.0, 2.4, "Fine", "S2"), (2.5, 3.0, "thanks", "S2")]
    json.dumps(out)
    rows = np.zeros((4, 8), np.int32)
    rows[:, 0], rows[:, 1], rows[:, 3] = [0, 0, 1, 1], [3, 2, 0, 5], [3, 4, 1, 5]
    assert wd.attributed_sentences(OPENAI, rows) == [
        {"speaker": 0, "start": 0.0, "end": 0.9, "text": "Hello there", "words": 2, "min_votes_share": 0.5},
        {"speaker": 1, "start": 2.0, "end": 3.0, "text": "Fine thanks", "words": 2, "min_votes_share": 0.0}]
    for bad in ({}, {"results": []}, {"words": [{"text": "x"}]}, {"segments": []}):
        with pytest.raises(ValueError, match="unknown transcript layout"):
            wd.transcript_words(bad)
