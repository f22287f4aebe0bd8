"""CPU checks of smooth.py: smooth_host against hand-worked tables, against the per-speaker loops of tests/smooth_ref.py on every shared
case and on seeded random tables, the canonical form, the conversions from seconds and every ValueError.  No GPU."""
from __future__ import annotations

import numpy as np
import pytest

import smooth_ref as SR
from conftest import sub

sm = sub("smooth")
LIB = sub("_lib")
CASES = SR.cases()


def one(table, K, fill, keep, cap=2):
    """smooth_host on one recording -> (table as lists, filled, dropped)."""
    out, tal = sm.smooth_host(np.asarray(table, np.int32).reshape(-1, 2), [0, len(table)], [0, K], fill, keep, cap)
    assert out.dtype == np.int32 and tal.dtype == np.int32 and tal.shape == (1, 2)
    return out.tolist(), int(tal[0, 0]), int(tal[0, 1])


def line(out, k=0):
    return "".join("#" if k in row else "." for row in out)


def test_symbol_is_bound():
    assert "sdk_smooth_turns" in LIB.SIGNATURES and "sdk_smooth_turns_workspace_bytes" in LIB.SIGNATURES
    assert sm.MAX_SMOOTH_FRAMES == SR.MAX == 1024 and sm.SMOOTH_BLOCK_FRAMES == SR.T


def test_a_gap_of_fill_is_filled_and_one_of_fill_plus_one_is_not():
    for fill in (1, 2, 5):
        pattern = "##" + "." * fill + "#" + "." * (fill + 1) + "##"
        out, filled, dropped = one(SR.solo(pattern), 1, fill, 0)
        assert line(out) == "##" + "#" * fill + "#" + "." * (fill + 1) + "##" and (filled, dropped) == (fill, 0)
    assert line(one(SR.solo("#.#..#"), 1, 0, 0)[0]) == "#.#..#"


def test_leading_trailing_and_boundary_gaps_are_not_filled():
    out, filled, _ = one(SR.solo("..##..#.."), 1, 4, 0)
    assert line(out) == "..#####.." and filled == 2
    # the same frames as two recordings: the pause now ends one recording and begins the next
    sp = SR.solo("..##..#..")
    out, tal = sm.smooth_host(sp, [0, 5, 9], [0, 1, 2], 4, 0, 2)
    assert line(out.tolist()) == "..##..#.." and tal.tolist() == [[0, 0], [0, 0]]
    out, tal = sm.smooth_host(SR.solo("#.#" + "#.#"), [0, 3, 3, 6], [0, 1, 1, 2], 1, 0, 2)       # an empty recording between two
    assert line(out.tolist()) == "######" and tal.tolist() == [[1, 0], [0, 0], [1, 0]]


def test_three_speakers_want_one_frame():
    crowd = [[2, -1], [0, 1], [-1, -1], [0, 1], [2, -1]]
    assert one(crowd, 3, 3, 0, cap=2) == ([[2, -1], [0, 1], [0, 1], [0, 1], [2, -1]], 2, 0)
    assert one(crowd, 3, 3, 0, cap=1) == ([[2, -1], [0, 1], [0, -1], [0, 1], [2, -1]], 1, 0)      # the frames that name two keep both


def test_a_filler_never_displaces_an_original():
    table = [[0, -1], [1, 2], [0, -1]]
    assert one(table, 3, 1, 0) == (table, 0, 0)
    assert one([[0, -1], [-1, 2], [0, -1]], 3, 1, 0) == ([[0, -1], [2, 0], [0, -1]], 1, 0)       # the original first, the filler behind it
    assert one([[0, -1], [2, -1], [0, -1]], 3, 1, 0, cap=1) == ([[0, -1], [2, -1], [0, -1]], 0, 0)   # exclusive stays exclusive


def test_a_run_of_keep_minus_one_is_dropped_and_a_run_of_keep_is_kept():
    for keep in (2, 3, 7):
        pattern = "." + "#" * (keep - 1) + ".." + "#" * keep + "."
        out, filled, dropped = one(SR.solo(pattern), 1, 0, keep)
        assert line(out) == "." + "." * (keep - 1) + ".." + "#" * keep + "." and (filled, dropped) == (0, keep - 1)
    assert one(SR.solo("#.#"), 1, 0, 1) == (SR.solo("#.#").tolist(), 0, 0) and one(SR.solo("#.#"), 1, 0, 0)[2] == 0
    # fill comes first: two runs of 2 with a pause of 1 are one run of 5
    assert line(one(SR.solo("##.##"), 1, 1, 5)[0]) == "#####" and line(one(SR.solo("##.##"), 1, 0, 5)[0]) == "....."
    # the frame's other speaker moves to the low slot, in order
    assert one([[0, 1], [1, -1], [1, -1]], 2, 0, 2) == ([[1, -1], [1, -1], [1, -1]], 0, 1)


def test_a_filled_gap_that_lost_a_frame_to_the_cap_leaves_two_runs():
    # speaker 2 pauses over frames 2 .. 4; frame 3 names 0 and 1 and has no room: the runs of 2 are frames 0 .. 2 and frame 4 .. 6
    table = [[2, -1], [2, -1], [-1, -1], [0, 1], [-1, -1], [2, -1], [2, -1]]
    out, filled, dropped = one(table, 3, 3, 0)
    assert line(out, 2) == "###.###" and filled == 2
    out, filled, dropped = one(table, 3, 3, 4)
    assert line(out, 2) == "......." and line(out, 0) == "......." and (filled, dropped) == (2, 8)  # each run of 3 is short of 4, so are 0's and 1's single frames
    table[6:] = [[2, -1], [2, -1]]
    out, filled, dropped = one(table, 3, 3, 4)
    assert line(out, 2) == "....####" and (filled, dropped) == (2, 5)                              # judged separately: 3 goes, 4 stays


def test_doubles_and_entries_that_name_nobody():
    table = [[1, 1], [-1, 1], [5, 1], [3, -9], [1, 3], [2, 2], [-1, -1], [0, 2]]
    want = [[1, -1], [1, -1], [1, -1], [-1, -1], [1, -1], [2, -1], [-1, -1], [0, 2]]
    assert one(table, 3, 0, 0) == (want, 0, 0)
    out, filled, dropped = one(table, 3, 1, 0)
    assert out == [[1, -1], [1, -1], [1, -1], [1, -1], [1, -1], [2, -1], [2, -1], [0, 2]] and filled == 2
    assert one(table, 0, 3, 0) == ([[-1, -1]] * 8, 0, 0)                                       # K = 0: nobody


@pytest.mark.parametrize("name", sorted(CASES))
def test_smooth_host_equals_the_loops_on_every_case(name):
    c = CASES[name]
    want, tal, crowded = SR.smooth_ref(c["sp"], c["frame_off"], c["cent_off"], c["fill"], c["keep"], c["cap"])
    SR.holds(c, want, tal, crowded)
    got, got_tal = sm.smooth_host(c["sp"], c["frame_off"], c["cent_off"], c["fill"], c["keep"], c["cap"])
    assert np.array_equal(got, want) and np.array_equal(got_tal, tal), (name, np.argwhere(got != want)[:4].tolist(), got_tal.tolist(), tal.tolist())


@pytest.mark.parametrize("seed", [31, 32, 33, 34, 35, 36])
def test_smooth_host_equals_the_loops_on_random_run_tables(seed):
    c = SR.random_pack(seed)
    want, tal, crowded = SR.smooth_ref(c["sp"], c["frame_off"], c["cent_off"], c["fill"], c["keep"], c["cap"])
    SR.holds(c, want, tal, crowded)
    got, got_tal = sm.smooth_host(c["sp"], c["frame_off"], c["cent_off"], c["fill"], c["keep"], c["cap"])
    assert np.array_equal(got, want) and np.array_equal(got_tal, tal), (seed, np.argwhere(got != want)[:4].tolist())
    other = sm.smooth_host(c["sp"], c["frame_off"], c["cent_off"], c["fill"], c["keep"], 3 - c["cap"])[0]
    assert np.array_equal(other, SR.smooth_ref(c["sp"], c["frame_off"], c["cent_off"], c["fill"], c["keep"], 3 - c["cap"])[0])


def test_the_cases_cover_fill_drop_and_a_crowded_frame():
    filled = dropped = crowded = 0
    for c in CASES.values():
        _, tal, cr = SR.smooth_ref(c["sp"], c["frame_off"], c["cent_off"], c["fill"], c["keep"], c["cap"])
        filled, dropped, crowded = filled + int(tal[:, 0].sum()), dropped + int(tal[:, 1].sum()), crowded + cr
    assert filled > 0 and dropped > 0 and crowded > 0


def test_zero_frames_give_the_canonical_form():
    rng = np.random.default_rng(5)
    sp = SR.run_table(rng, 400, 3, noise=0.3)
    out, tal = sm.smooth_host(sp, [0, 150, 400], [0, 3, 6], 0, 0, 2)
    assert not tal.any()
    for g, (row, got) in enumerate(zip(sp.tolist(), out.tolist())):
        want = []
        for x in row:
            if 0 <= x < 3 and x not in want:
                want.append(x)
        assert got == (want + [-1, -1])[:2], (g, row, got)
    assert np.array_equal(sm.smooth_host(out, [0, 150, 400], [0, 3, 6], 0, 0, 1)[0], out)     # a fixed point, whatever the cap
    assert np.array_equal(sm.canonical(sp[:150], 3), out[:150])


def test_conversions():
    assert sm.fill_frames_of(0) == 0 and sm.keep_frames_of(0) == 0 and sm.keep_frames_of(0.0) == 0
    # fill rounds down to whole frames: a pause is filled when it is no longer than the time
    assert sm.fill_frames_of(269 / 16000) == 0 and sm.fill_frames_of(270 / 16000) == 1 and sm.fill_frames_of(539.4 / 16000) == 1
    assert sm.fill_frames_of(539.5 / 16000) == 2                 # 539.5 samples round half up to 540: two frames
    assert sm.fill_frames_of(0.1) == 5 and sm.fill_frames_of(0.5) == 29
    # keep rounds up: a turn stays when it is no shorter than the time
    assert sm.keep_frames_of(1 / 16000) == 1 and sm.keep_frames_of(270 / 16000) == 1 and sm.keep_frames_of(270.5 / 16000) == 2
    assert sm.keep_frames_of(270.4 / 16000) == 1 and sm.keep_frames_of(0.4 / 16000) == 0
    assert sm.keep_frames_of(0.25) == 15
    # half a frame, and a frame and a half: fill goes down, keep goes up
    assert (sm.fill_frames_of(135 / 16000), sm.keep_frames_of(135 / 16000)) == (0, 1)
    assert (sm.fill_frames_of(405 / 16000), sm.keep_frames_of(405 / 16000)) == (1, 2)
    assert sm.fill_frames_of(1024 * 270 / 16000) == 1024 and sm.keep_frames_of(1024 * 270 / 16000) == 1024


def test_refusals():
    for bad in (-0.1, float("nan"), 1025 * 270 / 16000, 1e9, float("inf")):
        with pytest.raises(ValueError, match="min_duration_off"):
            sm.fill_frames_of(bad)
    for bad in (-0.1, float("nan"), (1024 * 270 + 1) / 16000, 1e9, float("inf")):
        with pytest.raises(ValueError, match="min_duration_on"):
            sm.keep_frames_of(bad)
    sp = SR.solo("#.#")
    for fill, keep, cap in ((1025, 0, 2), (0, 1025, 2), (-1, 0, 2), (0, -1, 2)):
        with pytest.raises(ValueError, match="frames, 0 .. 1024"):
            sm.smooth_host(sp, [0, 3], [0, 1], fill, keep, cap)
    for cap in (0, 3):
        with pytest.raises(ValueError, match="1 or 2 speakers per frame"):
            sm.smooth_host(sp, [0, 3], [0, 1], 1, 1, cap)
    with pytest.raises(ValueError, match="frame_off"):
        sm.smooth_host(sp, [0, 2], [0, 1], 1, 1, 2)
    with pytest.raises(ValueError, match="cent_off"):
        sm.smooth_host(sp, [0, 3], [0, 1, 2], 1, 1, 2)
    with pytest.raises(ValueError, match="smoothing="):
        sm.check_pairs("sweep", [])
    with pytest.raises(ValueError, match="smoothing="):
        sm.check_pairs("sweep", [(0.1,)])
    with pytest.raises(ValueError, match="min_duration_on"):
        sm.check_pairs("sweep", [(0.1, -1.0)])
    assert sm.check_pairs("sweep", None) is None and sm.check_pairs("sweep", [(0, 0), (0.5, 0.25)]) == [(0.0, 0.0, 0, 0), (0.5, 0.25, 29, 15)]


def test_result_fields_and_keywords_exist():
    import inspect
    dz, sc, bk = sub("diarize"), sub("score"), sub("backend")
    assert dz.DiarizationResult.smoothing is None and "smoothing" not in dz.DiarizationResult.__dataclass_fields__
    for fn in (dz.Diarizer.run, dz.Diarizer.run_many):
        p = inspect.signature(fn).parameters
        assert p["min_duration_off"].default == 0.0 and p["min_duration_on"].default == 0.0
    assert inspect.signature(dz.Diarizer.sweep).parameters["smoothing"].default is None
    assert [f for f in sc.SmoothSweepResult.__dataclass_fields__] == ["thresholds", "smoothing", "per_recording", "pooled", "best"]
    p = inspect.signature(bk.smooth_diarization).parameters
    assert list(p) == ["be", "results", "min_duration_off", "min_duration_on", "max_speakers"]
