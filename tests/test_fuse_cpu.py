"""CPU checks of the fusion of several diarizations (fuse.py): every step of the rule on a hand-worked case, fuse_host against the
loop-per-frame restatement of tests/fuse_ref.py on the same cases and on seeded random packs, identical hypotheses, a planted truth whose
fused table scores no worse than its best noisy copy, the rank weights, and every host-side refusal with the library out of reach.
Every comparison is exact integer equality."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import pytest

import fuse_ref as FR
from conftest import sub

fu = sub("fuse")
sc = sub("score")
sm = sub("smooth")


def both(masks, frame_off, K, weights=None, cap=2):
    """fuse_host's tables, after they are shown equal to the restatement's."""
    got = fu.fuse_host(masks, frame_off, K, weights, cap)
    want = FR.fuse_ref(masks.tolist(), frame_off, np.asarray(K).tolist(), weights, cap)
    assert FR.same(got, want) is None, FR.same(got, want)
    return got


def labels(out, K, R=1):
    """label_of as [h][r] lists."""
    off = np.concatenate([[0], np.cumsum(np.asarray(K).reshape(-1))])
    H = len(K)
    return [[out["label_of"][off[h * R + r]:off[h * R + r + 1]].tolist() for r in range(R)] for h in range(H)]


def test_rank_weights_are_the_stated_literals():
    want = [math.floor(65536 * (k + 1) ** -0.1) for k in range(8)]
    assert list(fu.FUSE_RANK_WEIGHTS) == want == FR.RANK_WEIGHTS
    assert fu.FUSE_RANK_WEIGHTS[0] == 65536 and all(a > b for a, b in zip(fu.FUSE_RANK_WEIGHTS, fu.FUSE_RANK_WEIGHTS[1:]))
    assert len(fu.FUSE_RANK_WEIGHTS) == fu.MAX_FUSE_HYPS == 8 and fu.FUSE_BLOCK_FRAMES == FR.B == 256
    # the neighbours of every floor are far from an integer: no rounding of pow can move a literal
    assert all(1e-6 < (65536 * (k + 1) ** -0.1) % 1 < 1 - 1e-6 for k in range(1, 8))


def test_pair_numbering():
    for H in range(2, 9):
        assert [fu.pair_index(a, b, H) for a, b in fu.pairs(H)] == list(range(H * (H - 1) // 2))
        assert fu.pairs(H) == FR.pair_list(H)


def test_half_way_count_rounds_up_and_the_cap_holds():
    """H = 2, equal weights, counts 1 and 2: n = floor((2 * 3 + 2) / 4) = 2.  A[0][0] = A[0][1] = 3: the tie goes to j = 0, speaker 1 of
    hypothesis 1 gets the new label 1."""
    masks, off, K = FR.pack([[[[0]] * 3, [[0, 1]] * 3]], [[1], [2]])
    out = both(masks, off, K, weights=[1, 1])
    assert labels(out, K) == [[[0]], [[0, 1]]] and out["n_labels"].tolist() == [2]
    assert out["speakers"].tolist() == [[0, 1]] * 3 and out["tallies"].tolist() == [[3, 3, 0, 0]]
    assert both(masks, off, K, weights=[1, 1], cap=1)["speakers"].tolist() == [[0, -1]] * 3
    masks, off, K = FR.pack([[[[0]] * 3, [[0]] * 3]], [[1], [2]])              # counts 1 and 1: n = 1
    assert both(masks, off, K, weights=[1, 1])["speakers"].tolist() == [[0, -1]] * 3


def test_vote_tie_goes_to_the_lower_label():
    a = [[0]] * 3 + [[1]] * 3 + [[1]]
    b = [[0]] * 3 + [[1]] * 3 + [[0]]
    masks, off, K = FR.pack([[a, b]], [[2], [2]])
    out = both(masks, off, K, weights=[7, 7])
    assert labels(out, K) == [[[0, 1]], [[0, 1]]]
    assert out["speakers"][6].tolist() == [0, -1]                               # v[0] = v[1] = 7, n = 1
    assert out["tallies"].tolist() == [[7, 0, 6, 0]]
    assert both(masks, off, K, weights=[7, 8])["speakers"][6].tolist() == [0, -1] and both(masks, off, K, weights=[8, 7])["speakers"][6].tolist() == [1, -1]


def test_greedy_tie_and_rank_tie():
    masks, off, K = FR.case_greedy_tie()
    out = both(masks, off, K)
    assert out["dis"][0].tolist() == [[0, 2], [2, 0]] and out["order"].tolist() == [[0, 1]]      # D_0 = D_1: the lower h is the anchor
    assert out["weight"].tolist() == [[fu.FUSE_RANK_WEIGHTS[0], fu.FUSE_RANK_WEIGHTS[1]]]
    assert out["co"].tolist() == [2, 2, 2, 0]
    assert labels(out, K) == [[[0, 1]], [[0, 2]]] and out["n_labels"].tolist() == [3]            # (0, 0) wins the three-way tie; A[1][1] = 0 maps nobody


def test_a_pair_is_read_transposed_when_the_higher_hypothesis_comes_first():
    masks, off, K = FR.case_transpose()
    out = both(masks, off, K)
    assert out["dis"][0].tolist() == [[0, 3, 2], [3, 0, 1], [2, 1, 0]] and out["order"].tolist() == [[2, 1, 0]]
    assert out["weight"][0].tolist() == [fu.FUSE_RANK_WEIGHTS[2], fu.FUSE_RANK_WEIGHTS[1], fu.FUSE_RANK_WEIGHTS[0]]
    assert labels(out, K) == [[[1, 0]], [[1, 0]], [[0, 1]]] and out["n_labels"].tolist() == [2]
    assert out["speakers"][:5, 0].tolist() == [1] * 5 and out["speakers"][6:12, 0].tolist() == [0] * 6
    assert both(masks, off, K, weights=[5, 1, 1])["weight"].tolist() == [[5, 1, 1]]


def test_label_overflow():
    masks, off, K = FR.case_overflow()
    out = both(masks, off, K)
    assert out["n_labels"].tolist() == [64] and out["overflow"].tolist() == [56] and out["tallies"][0, 3] == 56
    lab = labels(out, K)
    assert lab[0][0] == list(range(40)) and lab[1][0] == list(range(40, 64)) + [-1] * 16 and lab[2][0] == [-1] * 40
    # a frame whose only speaker has no label still counts one speaker (n = 0 here: one of three) and names nobody
    assert out["tallies"][0, 0] == 0 and out["tallies"][0, 2] == 120 - 64


def test_k_of_0_and_64_and_stray_bits():
    top = np.uint64(1) << np.uint64(63)
    masks = np.array([[top, top | np.uint64(1), np.uint64(1)], [np.uint64(1), top, top], [top, top, np.uint64(5)]], dtype=np.uint64)
    K = [[64], [1], [0]]                                                        # hypothesis 1 has speaker 0 only, hypothesis 2 nobody: their bit 63 is stray
    out = both(masks, [0, 3], K)
    assert out["tally"].tolist() == [[4, 1], [4, 0], [1, 0]] and out["co"][63] == 1 and out["co"][0] == 0 and out["co"].sum() == 1 and out["co"].shape == (64,)
    assert labels(out, K)[2] == [[]]
    out64 = both(np.array([[top] * 4, [top] * 4], dtype=np.uint64), [0, 4], [[64], [64]])
    assert out64["speakers"].tolist() == [[63, -1]] * 4 and out64["tallies"].tolist() == [[4, 0, 4, 63]]    # the 63 silent speakers of hypothesis 1 find no label left
    none = both(np.array([[top] * 2, [np.uint64(3)] * 2], dtype=np.uint64), [0, 2], [[0], [0]])
    assert none["n_labels"].tolist() == [0] and none["speakers"].tolist() == [[-1, -1]] * 2 and none["tallies"].tolist() == [[0, 0, 2, 0]]
    assert np.array_equal(fu.masks_host([[-1, 63], [64, 0], [2, 2], [5, 1]], 64), np.array([top, 1, 4, 34], dtype=np.uint64))
    assert fu.masks_host([[0, 1], [1, 1]], 1).tolist() == [1, 0] and fu.masks_host([[0, 1]], 0).tolist() == [0]
    assert FR.masks_ref([[-1, 63], [64, 0], [2, 2], [5, 1]], 64) == [1 << 63, 1, 4, 34]


def test_cap_on_a_frame_with_three_bits():
    a = [[0]] * 4 + [[1]] * 4 + [[2]] * 4 + [[0, 1, 2]]
    masks, off, K = FR.pack([[a, a, a]], [[3], [3], [3]])
    two, one = both(masks, off, K, cap=2), both(masks, off, K, cap=1)
    assert two["speakers"][12].tolist() == [0, 1] and one["speakers"][12].tolist() == [0, -1]
    assert two["tallies"].tolist() == [[13, 1, 13, 0]] and one["tallies"].tolist() == [[13, 0, 13, 0]]


@pytest.mark.parametrize("seed,H,frames", [(1, 2, [40, 0, 7]), (2, 3, [33, 64]), (3, 8, [25, 1, 30]), (4, 5, [120])])
def test_fuse_host_equals_the_restatement_on_random_packs(seed, H, frames):
    masks, off, K = FR.random_pack(seed, H, frames)
    both(masks, off, K)
    both(masks, off, K, weights=list(range(3, 3 + H)), cap=1)


def runs_table(rng, G, K=4, two=0.15):
    sp = np.full((G, 2), -1, np.int32)
    g = 0
    while g < G:
        n = int(rng.integers(5, 60))
        k = int(rng.integers(-1, K))
        sp[g:g + n, 0] = k
        if k >= 0 and rng.random() < two:
            sp[g + n // 2:g + n, 1] = (k + 1 + int(rng.integers(0, K - 1))) % K
        g += n
    return sp


def host_fuse(hypotheses, n_samples=None, weights=None, max_speakers=None):
    """fuse_results with fuse_host in the device's place."""
    pk = fu.prepare("fuse", hypotheses, n_samples)
    out = fu.fuse_host(fu.masks_of(pk), pk.tab.frame_off, pk.tab.K, fu.check_weights("fuse", weights, pk.H), fu._cap_of("fuse", max_speakers))
    return fu.assemble(pk, hypotheses, out)


def result(sp, K):
    return SimpleNamespace(speakers=np.asarray(sp, np.int32), n_speakers=K, turns=[], centroids=None)


@pytest.mark.parametrize("H", [2, 3, 8])
def test_identical_hypotheses_return_the_input(H):
    sp = runs_table(np.random.default_rng(H), 700)
    sp[20:24, 0], sp[30:34, 0], sp[40:44, 0], sp[50:54, 0] = 0, 1, 2, 3                  # every speaker speaks (a silent one would find no partner)
    sp[10] = [2, 2]
    sp[11] = [-1, 3]
    sp[12] = [9, 1]
    (res,) = host_fuse([[result(sp, 4) for _ in range(H)]])
    canon = sm.canonical(sp, 4)
    assert np.array_equal(np.sort(res.speakers, 1), np.sort(canon, 1)) and res.speakers.dtype == np.int32
    assert (res.speakers[:, 0] >= 0).sum() == (canon[:, 0] >= 0).sum()               # compacted to the low slot
    f = res.fusion
    assert not f["dis"].any() and f["unanimous"] == 700 and f["overflow"] == 0 and f["order"] == list(range(H))
    assert f["label_of"] == [{k: k for k in range(4)}] * H and res.n_speakers == 4
    assert f["speech"] == int((canon[:, 0] >= 0).sum()) and f["overlap"] == int((canon[:, 1] >= 0).sum())
    assert res.turns == sub("diarize_host").turns_from_frames(res.speakers, 4)


def truth_turns(sp, K):
    out = []
    for k in range(K):
        on = (sp == k).any(1)
        edge = np.diff(np.concatenate([[0], on.astype(np.int8), [0]]))
        out += [((270 * int(a) + 495) / 16000, (270 * int(b) + 495) / 16000, f"t{k}") for a, b in zip(np.nonzero(edge == 1)[0], np.nonzero(edge == -1)[0])]
    return out


PLANTED_SEED = 20


def test_planted_truth_is_recovered_no_worse_than_the_best_copy():
    G, K = 4000, 4
    rng = np.random.default_rng(PLANTED_SEED)
    truth = runs_table(rng, G, K)
    assert ((truth >= 0).sum(1) == 2).sum() > 50
    n = 270 * G + 226
    ref = truth_turns(truth, K)
    assert sc.score_host(truth, n, ref).der == 0.0
    copies = []
    for c in range(3):
        r2 = np.random.default_rng(1000 * PLANTED_SEED + c)
        sp = truth.copy()
        speech = np.nonzero(sp[:, 0] >= 0)[0]
        for g in r2.choice(speech, size=G // 10, replace=False):
            sp[g, 0] = r2.choice([k for k in range(K) if k not in sp[g]])
        perm = r2.permutation(K)
        copies.append(result(np.where(sp >= 0, perm[np.maximum(sp, 0)], -1), K))
    ders = [sc.score_host(c.speakers, n, ref).der for c in copies]
    (res,) = host_fuse([copies])
    fused = sc.score_host(res.speakers, n, ref).der
    print(f"planted truth: DER of the copies {[round(d, 4) for d in ders]}, fused {fused:.4f}, fusion {res.fusion['order']} {res.fusion['weights']}")
    assert min(ders) > 0.05 and fused <= min(ders)
    assert res.n_speakers == K and res.fusion["overflow"] == 0


def test_turn_lists_and_results_mix():
    sp = np.full((20, 2), -1, np.int32)
    sp[2:9, 0] = 0
    sp[12:18, 0] = 1
    turns = [((270 * 12 + 495) / 16000, (270 * 18 + 495) / 16000, "bob"), ((270 * 2 + 495) / 16000, (270 * 9 + 495) / 16000, "amy")]
    hyps = [[result(sp, 2), turns, turns]]
    (res,) = host_fuse(hyps)                                                    # G comes from the result
    assert res.fusion["label_of"][1] == {"amy": 0, "bob": 1} and res.fusion["unanimous"] == 20 and np.array_equal(res.speakers, sp)
    (only,) = host_fuse([[turns, turns]], n_samples=[270 * 20 + 226])
    assert isinstance(only, fu.FusedDiarization) and np.array_equal(only.speakers, sp) and only.n_speakers == 2
    assert only.turns == sub("diarize_host").turns_from_frames(sp, 2)


class Unreachable:
    def __getattr__(self, name):
        raise AssertionError(f"the engine was asked for {name}: the refusal must come before any library call")


def test_host_side_refusals_come_before_the_library():
    eng = Unreachable()
    a, b, short = result(np.full((5, 2), -1), 1), result(np.full((5, 2), -1), 2), result(np.full((4, 2), -1), 1)
    turns = [(0.0, 0.1, "x")]
    for bad, kw, what in [([[a, short]], {}, "frames"),
                          ([[a, b], [a, b, a]], {}, "same number of hypotheses"),
                          ([[a]], {}, "H=1"),
                          ([[a] * 9], {}, "H=9"),
                          ([[a, result(np.full((5, 2), -1), 65)]], {}, "65 speakers"),
                          ([[a, [(0.0, 1.0 + k, f"s{k}") for k in range(65)]]], {}, "65 speakers"),
                          ([[a, b]], {"weights": [1, 2, 3]}, "weights="),
                          ([[a, b]], {"weights": [0, 2]}, "weights="),
                          ([[a, b]], {"weights": [1, 65537]}, "weights="),
                          ([[a, b]], {"weights": [1.5, 2]}, "weights="),
                          ([[turns, turns]], {}, "n_samples"),
                          ([[a, b]], {"n_samples": [5]}, "frames"),
                          ([[a, b]], {"n_samples": [1, 2]}, "n_samples"),
                          ([[a, b]], {"max_speakers": -1}, "max_speakers"),
                          ([[a, 7]], {}, "a result")]:
        with pytest.raises(ValueError, match=what):
            fu.fuse_results(eng, bad, **kw)
    with pytest.raises(ValueError, match="frames"):
        fu.compare(eng, [a], [short])
    with pytest.raises(ValueError, match="1 and 2 hypotheses"):
        fu.compare(eng, [a], [a, b])
    assert fu.fuse_results(eng, []) == [] and fu.compare(eng, [], []) == []
    with pytest.raises(ValueError, match="cap="):
        fu.fuse_host(np.zeros((2, 1), np.uint64), [0, 1], [[1], [1]], cap=3)
    with pytest.raises(ValueError, match="H=9"):
        fu.fuse_host(np.zeros((9, 1), np.uint64), [0, 1], [[1]] * 9)
