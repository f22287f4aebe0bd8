"""CPU checks of the diarization error rate (score.py): the three new C-ABI symbols, the RTTM reader against diarize.to_rttm, known answers
worked by hand on a 10-s grid, score_host against the independent restatement tests/der_ref.py on seeded random cases, and the refusals."""
import math

import numpy as np
import pytest

import der_ref as DRF
from conftest import sub

LIB = sub("_lib")
sc = sub("score")
dz = sub("diarize")

NEW_SYMBOLS = ["sdk_score_reference", "sdk_score_cooccur", "sdk_score_map"]


def test_new_symbols_are_exported_and_bound():
    lib = LIB.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported by libsdk_hip.so"
        assert name in LIB.SIGNATURES
    assert lib.sdk_abi_version() == LIB.ABI_VERSION == 4                  # symbols are only added


def test_parse_rttm_reads_what_to_rttm_writes():
    turns = [(0.0, 1.23456, 0), (1.0, 2.0004, 1), (3.3333, 17.00049, 0), (20.5, 20.75, 11)]
    text = dz.to_rttm(turns, "rec-a") + "SPKR-INFO rec-a 1 <NA> <NA> <NA> unknown SPEAKER_00 <NA> <NA>\n\n" + dz.to_rttm(turns[:1], "rec-b")
    got = sc.parse_rttm(text)
    assert sorted(got) == ["rec-a", "rec-b"] and len(got["rec-a"]) == 4 and len(got["rec-b"]) == 1
    for (a, b, k), (ga, gb, name) in zip(turns, got["rec-a"]):
        # to_rttm rounds the start and the duration to 3 decimals each: the start comes back within 0.0005, the end within 0.001
        assert abs(ga - a) <= 0.0005 + 1e-9 and abs(gb - b) <= 0.001 + 1e-9 and name == f"SPEAKER_{k:02d}"
    assert sc.references_for(text, ["rec-b", "rec-a"])[1] == got["rec-a"]


# ------------------------------------------------------------------------------------------------ known answers, worked by hand
# 10 s = 160 000 samples: frames g = 0 .. 590 (270 * 590 + 495 = 159 795 < 160 000 <= 270 * 591 + 495), G = 591.  A turn boundary at 5 s =
# 80 000 samples: centres below it are g <= 294 (270 * 294 + 495 = 79 875), so [0, 5) s holds 295 frames and [5, 10) s holds 296.
N10 = 160000
G10 = 591
AB = [(0.0, 5.0, "A"), (5.0, 10.0, "B")]


def hyp_of(spans, G=G10):
    """[(first frame, end frame, speaker)] -> speakers [G, 2]: a frame's speakers in the order given."""
    sp = np.full((G, 2), -1, np.int32)
    for a, b, k in spans:
        for g in range(a, b):
            sp[g, 0 if sp[g, 0] < 0 else 1] = k
    return sp


def tallies_of(r):
    return (r.scored, r.total, r.missed, r.false_alarm, r.confusion, r.correct)


def test_known_answers():
    assert dz.global_frames(N10) == G10
    same = sc.score_host(hyp_of([(0, 295, 0), (295, 591, 1)]), N10, AB)
    assert tallies_of(same) == (591, 591, 0, 0, 0, 591) and same.der == 0.0 and same.mapping == {"A": 0, "B": 1}
    assert np.array_equal(same.co, [[295, 0], [0, 296]])
    perm = sc.score_host(hyp_of([(0, 295, 1), (295, 591, 0)]), N10, AB)
    assert tallies_of(perm) == (591, 591, 0, 0, 0, 591) and perm.der == 0.0 and perm.mapping == {"A": 1, "B": 0}
    miss = sc.score_host(hyp_of([(0, 295, 0)]), N10, AB)                   # B is never hypothesised: pure miss
    assert tallies_of(miss) == (591, 591, 296, 0, 0, 295) and miss.der == 296 / 591 and miss.mapping == {"A": 0, "B": -1}
    extra = sc.score_host(hyp_of([(0, 295, 0), (295, 591, 1), (0, 100, 2)]), N10, AB)      # a third speaker beside A on 100 frames: pure false alarm
    assert tallies_of(extra) == (591, 591, 0, 100, 0, 591) and extra.der == 100 / 591
    # B's 296 frames: the first 148 as speaker 1, the last 148 as speaker 0, which is A's: co = [[295, 0], [148, 148]], the best map is
    # A -> 0, B -> 1 with 295 + 148 = 443 correct, so 148 frames are confused
    swap = sc.score_host(hyp_of([(0, 295, 0), (295, 443, 1), (443, 591, 0)]), N10, AB)
    assert np.array_equal(swap.co, [[295, 0], [148, 148]])
    assert tallies_of(swap) == (591, 591, 0, 0, 148, 443) and swap.der == 148 / 591 and swap.mapping == {"A": 0, "B": 1}
    assert sc.score_host(np.zeros((0, 2), np.int32), 0, []).der == 0.0
    fa_only = sc.score_host(hyp_of([(0, 10, 0)]), N10, [])
    assert tallies_of(fa_only) == (591, 0, 0, 10, 0, 0) and fa_only.der == math.inf
    pooled = sc.pool([miss, extra])
    assert tallies_of(pooled) == (1182, 1182, 296, 100, 0, 886) and pooled.der == 396 / 1182 and pooled.mapping == {} and pooled.co is None
    assert abs(pooled.total_s - 1182 * 270 / 16000) < 1e-12


def test_collar_and_skip_overlap_remove_the_stated_frames():
    # A speaks 2 - 4 s = samples [32 000, 64 000): centres 270 g + 495 inside for g = 117 .. 235, 119 frames.  Collar 0.25 s = 4000 samples:
    # around 32 000 the centres in (28 000, 36 000) are g = 102 .. 131 (30 frames), around 64 000 those in (60 000, 68 000) are g = 221 .. 250
    # (30 frames).  591 - 60 = 531 frames stay, of which A holds 119 - 15 - 15 = 89 (g = 132 .. 220).
    ref = [(2.0, 4.0, "A")]
    hyp = hyp_of([(117, 236, 0)])
    plain = sc.score_host(hyp, N10, ref)
    assert tallies_of(plain) == (591, 119, 0, 0, 0, 119)
    col = sc.score_host(hyp, N10, ref, collar_s=0.25)
    assert tallies_of(col) == (531, 89, 0, 0, 0, 89) and col.der == 0.0
    late = sc.score_host(hyp_of([(125, 236, 0)]), N10, ref)               # the hypothesis starts 8 frames late: a miss that the collar forgives
    assert tallies_of(late)[:3] == (591, 119, 8) and sc.score_host(hyp_of([(125, 236, 0)]), N10, ref, collar_s=0.25).der == 0.0
    # A 0 - 6 s, B 4 - 10 s: both in samples [64 000, 96 000), g = 236 .. 353, 118 frames that skip_overlap removes
    two = [(0.0, 6.0, "A"), (4.0, 10.0, "B")]
    hyp2 = hyp_of([(0, 354, 0), (236, 591, 1)])
    full = sc.score_host(hyp2, N10, two)
    assert tallies_of(full) == (591, 591 + 118, 0, 0, 0, 591 + 118)
    skip = sc.score_host(hyp2, N10, two, skip_overlap=True)
    assert tallies_of(skip) == (473, 473, 0, 0, 0, 473)
    # with the collar too: boundaries at 0 s (g = 0 .. 12), 4 s (g = 221 .. 250), 6 s (g = 339 .. 368) and 10 s (g = 576 .. 590); with the
    # overlap g = 236 .. 353 the frames 221 .. 368 go as one run: 13 + 148 + 15 = 176 frames are not scored
    both = sc.score_host(hyp2, N10, two, collar_s=0.25, skip_overlap=True)
    assert both.scored == 591 - 176 and both.der == 0.0


# ------------------------------------------------------------------------------------------------ against the independent restatement
CASES = [(S, K, n) for n in (0, 400, 495, 496, 5 * 16000, 23 * 16000 + 333) for S, K in ((0, 0), (1, 3), (3, 1), (3, 3), (64, 3), (3, 64), (0, 3), (3, 0))] + \
        [(64, 64, 5 * 16000), (64, 64, 23 * 16000 + 333), (1, 1, 496)]


@pytest.mark.parametrize("collar_s,skip", [(0.0, False), (0.25, False), (0.0, True), (0.25, True)])
def test_score_host_equals_the_restatement(collar_s, skip):
    rng = np.random.default_rng(2601)
    seen = set()
    for S, K, n in CASES:
        turns = DRF.random_turns(rng, S, n)
        G = DRF.n_frames(n)
        assert G == dz.global_frames(n)
        sp = DRF.random_speakers(rng, G, K)
        want = DRF.der_ref(sp, n, turns, collar_s, skip)
        got = sc.score_host(sp, n, turns, collar_s, skip)
        assert list(got.mapping) == want["names"]
        assert tallies_of(got) == (want["scored"], want["total"], want["missed"], want["false_alarm"], want["confusion"], want["correct"]), (S, K, n)
        assert np.array_equal(got.co, want["co"]) and got.der == want["der"]
        m = [got.mapping[nm] for nm in want["names"]]
        used = [j for j in m if j >= 0]
        assert len(set(used)) == len(used) and sum(int(got.co[i, j]) for i, j in enumerate(m) if j >= 0) == got.correct
        assert all(got.co[i, j] > 0 for i, j in enumerate(m) if j >= 0)
        merged, names = sc.prepare_reference(turns)
        mask, scored = sc.reference_masks_host(merged, G, sc.collar_samples(collar_s), skip)
        assert [int(v) for v in mask] == want["mask"] and [bool(v) for v in scored] == want["scored_frames"]
        seen.add((want["total"] > 0, want["confusion"] > 0, want["scored"] < G))
    assert (True, True, False) in seen or (True, True, True) in seen      # the cases reach real confusion


def test_assignment_host_is_exact():
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(5)
    for S, K in ((1, 1), (1, 64), (64, 1), (3, 5), (37, 64), (64, 64), (0, 4), (4, 0)):
        for co in (rng.integers(0, 1 << 20, (S, K)), rng.integers(0, 2, (S, K)), np.zeros((S, K), np.int64), rng.integers((1 << 30) - 64, 1 << 30, (S, K))):
            m, correct = sc.assignment_host(co)
            r, c = linear_sum_assignment(co, maximize=True)
            assert correct == int(co[r, c].sum())
            used = m[m >= 0]
            assert len(set(used.tolist())) == len(used) and sum(int(co[i, j]) for i, j in enumerate(m) if j >= 0) == correct


def test_preparation_rules():
    merged, names = sc.prepare_reference([(3.0, 4.0, "b"), (1.0, 2.0, "z"), (2.0, 2.5, "z"), (1.0, 1.5, "a"), (1.2, 1.1, "a"), (7.0, 7.0, "q"), (0.99999, 1.00001, "m")])
    assert names == ["a", "m", "z", "b", "q"]                             # by first start in samples (1.0 s and 0.99999 s are both 16 000), then by name
    assert merged.tolist() == [[16000, 24000, 0], [16000, 40000, 2], [48000, 64000, 3]]
    assert sc.to_samples(0.00003125) == 1 and sc.to_samples(0.000031) == 0   # floor(t * 16000 + 0.5)


def test_refusals():
    sp = np.full((dz.global_frames(16000), 2), -1, np.int32)
    many = [(0.1 * i, 0.1 * i + 0.05, f"s{i}") for i in range(65)]
    with pytest.raises(ValueError, match="at most 64"):
        sc.score_host(sp, 16000, many)
    sp65 = sp.copy()
    sp65[0, 0] = 64
    with pytest.raises(ValueError, match="at most 64"):
        sc.score_host(sp65, 16000, [])
    with pytest.raises(ValueError, match="frames"):
        sc.score_host(sp[:-1], 16000, [])
    with pytest.raises(ValueError, match="time"):
        sc.prepare_reference([(-1.0, 2.0, "a")])
    with pytest.raises(ValueError, match="collar_s"):
        sc.score_host(sp, 16000, [], collar_s=-0.1)
    with pytest.raises(ValueError, match="no uri"):
        sc.references_for(dz.to_rttm([(0.0, 1.0, 0)], "here"), ["here", "missing"])
    d = dz.Diarizer(None, None, None)
    # no engine is touched below: every refusal comes before the device
    one = dz.DiarizationResult([], 0, np.zeros((0, 4), np.float32), np.zeros((0, 3), np.int32), np.zeros(0, np.uint8), np.full((0, 2), -1, np.int32),
                               np.zeros(0, np.int64), np.zeros((0, 3, 4), np.int32))
    with pytest.raises(ValueError, match="2 references for 1 recordings"):
        d.score([one], [[], []])
    x = np.zeros(16000, np.int16)
    with pytest.raises(ValueError, match="2 references for 1 recordings"):
        d.sweep([x], [[], []], [0.5])
    with pytest.raises(ValueError, match="clustering='vbx'"):
        d.sweep([x], [[]], [0.5], clustering="vbx")
    with pytest.raises(ValueError, match="speakers=2"):
        d.sweep([x], [[]], [0.5], speakers=2)
    with pytest.raises(ValueError, match="thresholds"):
        d.sweep([x], [[]], [])
