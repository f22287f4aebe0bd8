"""CPU checks of scoring the DIHARD way (score.py): the evaluation map (UEM) at frame centres, the UEM reader, the integer Jaccard table and
the Jaccard error rate against brute force, exact rationals and scipy, the overflow and degenerate cases, pooling, purity and coverage by
hand, and that nothing changes with the new keywords at their defaults."""
import dataclasses
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import der_ref as DRF
from conftest import sub

LIB = sub("_lib")
sc = sub("score")
dz = sub("diarize")

NEW_SYMBOLS = ["sdk_score_uem", "sdk_score_durations", "sdk_score_jaccard"]
RATE, HOP, FIRST = 16000, 270, 495
ONE = 1 << 30


def secs(sample: int) -> float:
    t = sample / RATE
    assert sc.to_samples(t) == sample
    return t


def centre(g: int) -> int:
    return HOP * g + FIRST


def eligible(uem, G):
    return sc.uem_mask_host(sc.prepare_uem(uem), G).tolist()


def test_new_symbols_are_exported_and_bound():
    lib = LIB.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported by libsdk_hip.so"
        assert name in LIB.SIGNATURES
    assert lib.sdk_abi_version() == LIB.ABI_VERSION == 4                  # symbols are only added


# ------------------------------------------------------------------------------------------------ the evaluation map
def test_uem_mask_at_frame_centres():
    G = 10
    on = lambda *gs: [int(g in gs) for g in range(G)]  # noqa: E731
    assert eligible([(secs(centre(3)), secs(centre(6)))], G) == on(3, 4, 5)              # starts on a centre: in; ends on a centre: out
    assert eligible([(secs(centre(3) + 1), secs(centre(6) + 1))], G) == on(4, 5, 6)      # one sample past either centre
    assert eligible([(secs(centre(3) + 1), secs(centre(4)))], G) == on()                 # holds no centre
    assert eligible([(secs(centre(2)), secs(centre(4))), (secs(centre(4)), secs(centre(5)))], G) == on(2, 3, 4)       # abutting
    assert sc.prepare_uem([(secs(centre(2)), secs(centre(4))), (secs(centre(4)), secs(centre(5)))]).tolist() == [[centre(2), centre(5)]]
    over = [(secs(centre(7)), secs(centre(9))), (secs(centre(1)), secs(centre(3))), (secs(centre(2)), secs(centre(8))), (secs(4000), secs(4000)),
            (secs(5000), secs(4990))]
    assert sc.prepare_uem(over).tolist() == [[centre(1), centre(9)]]                     # overlapping, unsorted; empty and reversed intervals go
    assert eligible(over, G) == on(1, 2, 3, 4, 5, 6, 7, 8)
    assert eligible(None, G) == [1] * G and eligible([], G) == [0] * G                   # None and [] are different things
    assert sc.prepare_uem(None).tolist() == [[0, (1 << 31) - 1]] and sc.prepare_uem([]).shape == (0, 2)
    assert eligible([(secs(centre(8)), 1000.0)], G) == on(8, 9)                          # past the recording's end
    assert eligible([(50.0, 60.0)], G) == on() and eligible([(0.0, 1.0)], 0) == []
    with pytest.raises(ValueError, match="time"):
        sc.prepare_uem([(-1.0, 2.0)])


def test_parse_uem_and_uems_for(tmp_path):
    text = "; a comment\nrec-a 1 0.000 10.5\n\nrec-b 1 2 3\n  rec-a 1 20 30.25 trailing\n;rec-c 1 0 1\n"
    got = sc.parse_uem(text)
    assert got == {"rec-a": [(0.0, 10.5), (20.0, 30.25)], "rec-b": [(2.0, 3.0)]}
    assert sc.uems_for(text, ["rec-b", "missing", "rec-a"]) == [[(2.0, 3.0)], None, [(0.0, 10.5), (20.0, 30.25)]]
    path = tmp_path / "dev.uem"
    path.write_text(text)
    assert sc.uems_for(path, ["rec-b"]) == [[(2.0, 3.0)]] and sc.uems_for(str(path), ["x"]) == [None]
    assert sc.uems_for({"a": []}, ["a", "b"]) == [[], None]
    with pytest.raises(ValueError, match="line 2"):
        sc.parse_uem("a 1 0 1\nb 1 0\n")
    with pytest.raises(ValueError, match="line 3"):
        sc.parse_uem("a 1 0 1\n\nb 1 zero 4\n")
    assert sc.resolve_uems("t", None, None, 3) is None and sc.resolve_uems("t", [None, []], None, 2) == [None, []]
    assert sc.resolve_uems("t", text, ["rec-b", "q"], 2) == [[(2.0, 3.0)], None]
    with pytest.raises(ValueError, match="needs uris"):
        sc.resolve_uems("t", text, None, 2)
    with pytest.raises(ValueError, match="1 UEM entries for 2"):
        sc.resolve_uems("t", [None], None, 2)


# ------------------------------------------------------------------------------------------------ the Jaccard table and the JER
def random_tables(rng, S, K):
    """A co table with the durations of some frame set behind it: co <= min(ref, hyp) cell by cell, zero rows and columns now and then."""
    co = rng.integers(0, 400, (S, K)) * (rng.uniform(size=(S, K)) < 0.7)
    ref = co.sum(1) + rng.integers(0, 300, S) * (rng.uniform(size=S) < 0.8)
    hyp = co.sum(0) + rng.integers(0, 300, K) * (rng.uniform(size=K) < 0.8)
    return co.astype(np.int64), ref.astype(np.int64), hyp.astype(np.int64)


def injective_maps(S, K):
    """Every map of some reference speakers to pairwise different hypothesis speakers, as tuples with -1 for unmapped."""
    for cols in itertools.product(range(-1, K), repeat=S):
        used = [j for j in cols if j >= 0]
        if len(set(used)) == len(used):
            yield cols


def test_jaccard_table_and_jer_against_brute_force_fractions_and_scipy():
    rng = np.random.default_rng(3601)
    seen_silent = False
    for S, K in [(s, k) for s in range(1, 6) for k in range(1, 6)] + [(5, 5)] * 5:
        co, ref, hyp = random_tables(rng, S, K)
        q = sc.jaccard_table_host(co, ref, hyp)
        assert q.dtype == np.int32 and q.shape == (S, K) and q.min() >= 0 and q.max() <= ONE
        exact = [[Fraction(int(co[i, j]), int(ref[i] + hyp[j] - co[i, j])) if co[i, j] else Fraction(0) for j in range(K)] for i in range(S)]
        for i in range(S):
            for j in range(K):
                assert int(q[i, j]) == math.floor(exact[i][j] * ONE) and 0 <= exact[i][j] - Fraction(int(q[i, j]), ONE) < Fraction(1, ONE)
        mapping, jsum = sc.assignment_host(q)
        maps = list(injective_maps(S, K))
        assert jsum == max(sum(int(q[i, j]) for i, j in enumerate(m) if j >= 0) for m in maps)
        assert sum(int(q[i, j]) for i, j in enumerate(mapping) if j >= 0) == jsum
        Sp = int((ref > 0).sum())
        jer = sc.jer_value(jsum, Sp, bool((hyp > 0).any()))
        if Sp == 0:
            continue
        best = max(sum((exact[i][j] for i, j in enumerate(m) if j >= 0), Fraction(0)) for m in maps)
        assert abs(Fraction(jer) - (1 - best / Sp)) <= Fraction(1, ONE), (S, K)
        J = np.array([[float(x) for x in row] for row in exact])
        rows, cols = linear_sum_assignment(J, maximize=True)
        assert abs(jer - (1.0 - J[rows, cols].sum() / Sp)) <= 1e-9, (S, K)
        seen_silent |= Sp < S
    assert seen_silent                                                       # a reference speaker without frames was among the cases


def test_jaccard_overflow_cases():
    big = (1 << 31) - 1
    assert sc.jaccard_table_host([[1]], [big], [big]).tolist() == [[(1 << 30) // (2 * big - 1)]] == [[0]]
    q = sc.jaccard_table_host([[big]], [big], [big])
    assert q.dtype == np.int32 and q.tolist() == [[ONE]]                  # numerator (2^31 - 1) 2^30 ~ 2^61: exactly one
    assert sc.jaccard_table_host([[big // 2]], [big], [big]).tolist() == [[((big // 2) << 30) // (2 * big - big // 2)]]   # denominator past 2^31
    assert sc.assignment_host(q)[1] == ONE and sc.jer_value(ONE, 1) == 0.0


# 10 s = 160 000 samples, G = 591; [0, 5) s holds frames 0 .. 294, [5, 10) s frames 295 .. 590 (tests/test_der_cpu.py)
N10, G10 = 160000, 591
AB = [(0.0, 5.0, "A"), (5.0, 10.0, "B")]


def hyp_of(spans, G=G10):
    sp = np.full((G, 2), -1, np.int32)
    for a, b, k in spans:
        for g in range(a, b):
            sp[g, 0 if sp[g, 0] < 0 else 1] = k
    return sp


def test_jer_known_answers_and_degenerate_cases():
    same = sc.score_host(hyp_of([(0, 295, 0), (295, 591, 1)]), N10, AB, jer=True)
    assert (same.jer, same.jsum, same.ref_speakers, same.purity, same.coverage) == (0.0, 2 * ONE, 2, 1.0, 1.0)
    assert same.ref_frames.tolist() == [295, 296] and same.hyp_frames.tolist() == [295, 296] and same.jer_mapping == {"A": 0, "B": 1}
    # B's frames: the first 148 as speaker 1, the last 148 as speaker 0 (A's): co = [[295, 0], [148, 148]], hyp_frames = [443, 148].
    # Jaccard: A-0 295 / (295 + 443 - 295) = 295/443, B-0 148 / (296 + 443 - 148) = 148/591, B-1 148 / (296 + 148 - 148) = 1/2
    swap = sc.score_host(hyp_of([(0, 295, 0), (295, 443, 1), (443, 591, 0)]), N10, AB, jer=True)
    assert swap.hyp_frames.tolist() == [443, 148] and swap.jer_mapping == {"A": 0, "B": 1}
    assert swap.jsum == (295 * ONE) // 443 + ONE // 2 and swap.ref_speakers == 2
    assert abs(swap.jer - (1 - (295 / 443 + 0.5) / 2)) <= 2.0 ** -30
    assert swap.coverage == (295 + 148) / 591 and swap.purity == (295 + 148) / 591
    # S' == 0, both ways
    quiet = sc.score_host(hyp_of([]), N10, [], jer=True)
    assert (quiet.jer, quiet.jsum, quiet.ref_speakers, quiet.purity, quiet.coverage) == (0.0, 0, 0, 1.0, 1.0) and quiet.jer_mapping == {}
    fa_only = sc.score_host(hyp_of([(0, 10, 0)]), N10, [], jer=True)
    assert (fa_only.jer, fa_only.jsum, fa_only.ref_speakers) == (1.0, 0, 0) and fa_only.hyp_frames.tolist() == [10] and fa_only.purity == 0.0
    # K == 0: every reference speaker is missed
    k0 = sc.score_host(hyp_of([]), N10, AB, jer=True)
    assert (k0.jer, k0.jsum, k0.ref_speakers, k0.coverage, k0.purity) == (1.0, 0, 2, 0.0, 1.0) and k0.hyp_frames.shape == (0,)
    assert k0.jer_mapping == {"A": -1, "B": -1}
    # the UEM [0, 5) s silences B: it leaves S' and is not mapped, and speaker 1 of the hypothesis holds no scored frame
    half = sc.score_host(hyp_of([(0, 295, 0), (295, 591, 1)]), N10, AB, uem=[(0.0, 5.0)], jer=True)
    assert (half.scored, half.total, half.missed, half.false_alarm, half.confusion) == (295, 295, 0, 0, 0) and half.der == 0.0
    assert half.ref_frames.tolist() == [295, 0] and half.hyp_frames.tolist() == [295, 0] and half.ref_speakers == 1
    assert half.jer == 0.0 and half.jsum == ONE and half.jer_mapping == {"A": 0, "B": -1} and half.mapping == {"A": 0, "B": -1}
    none = sc.score_host(hyp_of([(0, 295, 0)]), N10, AB, uem=[], jer=True)                 # an empty map scores nothing
    assert (none.scored, none.total, none.der, none.jer, none.ref_speakers) == (0, 0, 0.0, 0.0, 0)
    # the collar measures from the reference boundaries whatever the UEM: 0.25 s around 5 s removes frames 281 .. 309 + 1
    col = sc.score_host(hyp_of([(0, 295, 0), (295, 591, 1)]), N10, AB, collar_s=0.25, uem=[(4.0, 6.0)])
    plain = sc.score_host(hyp_of([(0, 295, 0), (295, 591, 1)]), N10, AB, collar_s=0.25)
    merged, _ = sc.prepare_reference(AB)
    _, scored = sc.reference_masks_host(merged, G10, 4000, False)
    assert col.scored == int((scored & sc.uem_mask_host(sc.prepare_uem([(4.0, 6.0)]), G10)).sum()) < plain.scored
    assert col.scored == sum(1 for g in range(G10) if 64000 <= centre(g) < 96000 and abs(centre(g) - 80000) >= 4000)


def test_defaults_change_nothing():
    rng = np.random.default_rng(3602)
    for S, K, n in ((3, 3, 5 * RATE), (0, 3, 400), (5, 2, 23 * RATE + 333), (64, 3, 5 * RATE)):
        turns, sp = DRF.random_turns(rng, S, n), DRF.random_speakers(rng, DRF.n_frames(n), K)
        for collar_s, skip in ((0.0, False), (0.25, True)):
            want = DRF.der_ref(sp, n, turns, collar_s, skip)
            old, new = sc.score_host(sp, n, turns, collar_s, skip), sc.score_host(sp, n, turns, collar_s, skip, uem=None, jer=False)
            for f in dataclasses.fields(sc.DerResult):
                a, b = getattr(old, f.name), getattr(new, f.name)
                assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, f.name
            assert [f.name for f in dataclasses.fields(sc.DerResult)][:9] == ["scored", "total", "missed", "false_alarm", "confusion", "correct", "der", "mapping", "co"]
            assert all(getattr(new, f.name) is None for f in dataclasses.fields(sc.DerResult)[9:])
            assert (new.scored, new.total, new.missed, new.false_alarm, new.confusion, new.correct) == \
                (want["scored"], want["total"], want["missed"], want["false_alarm"], want["confusion"], want["correct"]) and new.der == want["der"]
            # the DER part of a jer=True result is the same too, and a map that covers everything is no map
            full = sc.score_host(sp, n, turns, collar_s, skip, uem=[(0.0, 1000.0)], jer=True)
            assert (full.scored, full.total, full.missed, full.false_alarm, full.confusion, full.correct, full.der, full.mapping) == \
                (new.scored, new.total, new.missed, new.false_alarm, new.confusion, new.correct, new.der, new.mapping) and np.array_equal(full.co, new.co)
    assert sc.DerResult(1, 2, 3, 4, 5, 6, 0.5, {}, None).jer is None     # positional construction keeps working


def test_purity_and_coverage_by_hand():
    co = np.array([[5, 1], [2, 7], [0, 3]])
    ref, hyp = np.array([8, 9, 3]), np.array([10, 12])
    # coverage: row maxima 5 + 7 + 3 = 15 of 20 reference frames; purity: column maxima 5 + 7 = 12 of 22 hypothesis frames
    assert sc.purity_coverage(co, ref, hyp) == (12 / 22, 15 / 20)
    assert sc.purity_coverage(np.zeros((0, 2), int), np.zeros(0, int), np.array([4, 0])) == (0.0, 1.0)
    assert sc.purity_coverage(np.zeros((2, 0), int), np.array([4, 0]), np.zeros(0, int)) == (1.0, 0.0)


def test_pooled_figures_are_ratios_of_sums():
    swap = sc.score_host(hyp_of([(0, 295, 0), (295, 443, 1), (443, 591, 0)]), N10, AB, jer=True)
    k0 = sc.score_host(hyp_of([]), N10, AB + [(2.0, 3.0, "C")], jer=True)
    quiet = sc.score_host(hyp_of([]), N10, [], jer=True)
    fa_only = sc.score_host(hyp_of([(0, 10, 0)]), N10, [], jer=True)
    p = sc.pool([swap, k0, quiet])
    assert p.jsum == swap.jsum and p.ref_speakers == 5 and p.jer == 1.0 - swap.jsum / (ONE * 5) and p.jer_mapping == {} and p.ref_frames is None
    # C speaks in samples [32 000, 48 000): frames 117 .. 175, so k0's references hold 295 + 296 + 59 = 650 frames and cover none
    assert k0.ref_frames.tolist() == [295, 59, 296] and p.pc_sums == (443, 591, 443, 591 + 650)
    assert p.purity == 443 / 591 and p.coverage == 443 / 1241 and p.der == (148 + 650) / 1241
    assert sc.pool([quiet, quiet]).jer == 0.0 and sc.pool([quiet, fa_only]).jer == 1.0 and sc.pool([quiet, fa_only]).ref_speakers == 0
    assert sc.pool([sc.pool([swap, k0]), sc.pool([quiet])]).jer == p.jer                      # pooled results pool again
    plain = sc.score_host(hyp_of([]), N10, AB)
    mixed = sc.pool([swap, plain])                                                          # one result without the Jaccard part: none pooled
    assert mixed.jer is None and mixed.jsum is None and mixed.purity is None and mixed.total == swap.total + plain.total
    old = sc.pool([plain, plain])
    assert old == sc.DerResult(1182, 1182, 1182, 0, 0, 0, 1.0, {}, None)


def test_best_threshold_follows_the_metric():
    def res(der, jer):
        return sc.DerResult(0, 0, 0, 0, 0, 0, der, {}, None, jer=jer)
    pooled = [res(0.3, 0.1), res(0.2, 0.4), res(0.2, 0.1)]
    ths = [0.5, 0.9, 0.6]
    assert sc.best_threshold(ths, pooled) == sc.best_threshold(ths, pooled, "der") == 2      # 0.2 twice: nearer 0.7046
    assert sc.best_threshold(ths, pooled, "jer") == 2 and sc.best_threshold(ths[:2], pooled[:2], "jer") == 0
    with pytest.raises(ValueError, match="metric"):
        sc.check_metric("sweep", "purity")
    d = dz.Diarizer(None, None, None)
    x = np.zeros(16000, np.int16)
    with pytest.raises(ValueError, match="metric"):
        d.sweep([x], [[]], [0.5], metric="purity")                        # before the device
    with pytest.raises(ValueError, match="2 UEM entries for 1"):
        d.sweep([x], [[]], [0.5], uem=[None, None])
