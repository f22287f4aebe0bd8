"""The resampler's references and fixtures, on a machine without a GPU: the vectorised oracle (oracle/resample.py) equals the scalar
Python-integer evaluation of the documented formula (tests/resample_ref.py); sdk_resample_plan puts every row of the case table on the kernel
instantiation the table claims, and all four are reached; and every condition the GPU tests (tests/test_resample_paths_gpu.py) rely on holds
on the reference alone - a fixture that stops saturating, stops landing on a rounding tie or stops telling floor from truncation fails here."""
import numpy as np
import pytest

import resample_ref as rr
from conftest import sub
from oracle import resample as ors

LIB = sub("_lib")


def _check_all(x, taps, L, M):
    want = ors.resample_s16(x, np.asarray(taps, dtype=np.int32), L, M)
    assert len(want) == rr.out_len(len(x), L, M)
    assert want.tolist() == rr.resample_at(x, taps, L, M, range(len(want)))


@pytest.mark.parametrize("shape", rr.SYNTHETIC, ids=rr.case_id)
@pytest.mark.parametrize("ch", rr.CHANNELS)
def test_oracle_equals_scalar_reference_synthetic(shape, ch):
    L, M, K = shape
    taps = rr.synthetic_taps(L, M, K)
    for n_in in (1, 2, 7, 300 if L <= M else 30):                    # L / M = 1367 outputs per input sample on the interpolating row
        _check_all(rr.noise(n_in, ch, [L, M, K, ch, n_in]), taps, L, M)


@pytest.mark.parametrize("rate,n_in", [(8000, 300), (11025, 300), (44100, 300), (352800, 300), (352800, 3001)])
@pytest.mark.parametrize("ch", rr.CHANNELS)
def test_oracle_equals_scalar_reference_designed(rate, n_in, ch):
    taps, L, M, K = ors.design_taps(rate, 16000)
    _check_all(rr.noise(n_in, ch, [rate, ch, n_in]), taps, L, M)
    if ch == 1:                                                      # [n] and [n, 1] are the same signal
        x = rr.noise(n_in, 1, [rate, 1, n_in])
        assert ors.resample_s16(x[:, 0], taps, L, M).tolist() == rr.resample_at(x, taps, L, M, range(rr.out_len(n_in, L, M)))


def test_plan_reaches_all_four_instantiations():
    lib = LIB.load_library()
    got = {}
    for (L, M, K), rate, lds_taps, lds_win in rr.CASES:
        want = (1 if lds_taps else 0) | (2 if lds_win else 0)
        assert rr.plan_bits(L, M, K) == want, (L, M, K)              # the table agrees with the rule as stated
        got[(L, M, K)] = lib.sdk_resample_plan(L, M, K)
        assert got[(L, M, K)] == want, (L, M, K, got[(L, M, K)])
        if rate is not None:                                         # the designed rows are what the host design gives for that rate
            assert sub("resample").design_taps(rate, 16000)[1:] == (L, M, K) == ors.design_taps(rate, 16000)[1:]
    assert set(got.values()) == {0, 1, 2, 3}
    # the limits themselves: one byte group either side
    assert lib.sdk_resample_plan(2, 3, 8192) & 1 and not lib.sdk_resample_plan(2, 3, 8194) & 1          # 65536 B, 65552 B
    assert lib.sdk_resample_plan(1, 16, 14) & 2 and not lib.sdk_resample_plan(1, 16, 16) & 2            # 65536 B, 65540 B
    # the rates the older tests use stay where the issue found them
    for rate, want in ((8000, 3), (48000, 3), (44100, 3), (96000, 3), (11025, 2)):
        _, L, M, K = ors.design_taps(rate, 16000)
        assert lib.sdk_resample_plan(L, M, K) == want, rate
    # refused shapes
    for L, M, K in ((0, 1, 2), (1, 0, 2), (1, 1, 0), (1, 1, 1), (1, 1, 3), (-1, 1, 2), (1, -1, 2), (1, 1, -2), ((1 << 21) + 1, 1, 2), (1 << 30, 1, 4)):
        assert lib.sdk_resample_plan(L, M, K) == -1, (L, M, K)
    assert lib.sdk_resample_plan(1 << 21, 1, 2) == 2                 # L * K = 2^22 exactly is served (taps global, window in LDS)


@pytest.mark.parametrize("shape", rr.SATURATION, ids=rr.case_id)
def test_saturation_fixture_leaves_the_s16_range_on_both_sides(shape):
    L, M, K = shape
    rate = dict(rr.DESIGNED).get(shape)
    taps = ors.design_taps(rate, 16000)[0] if rate else rr.synthetic_taps(L, M, K)
    x, targets = rr.saturation_input(taps, L, M)
    raw = rr.resample_raw_at(x, taps, L, M, targets)
    h = taps.astype(np.int64)
    for j, (n, v) in enumerate(zip(targets, raw)):
        ph = n * M % L
        full = n * M // L - (K // 2 - 1) >= 0                        # the whole window is inside the signal (not so for target 0)
        if full:
            assert v == rr.round_shift((1 if j % 2 == 0 else -1) * 32767 * int(np.abs(h[ph]).sum())), (j, n)
    assert sum(v > 32767 for v in raw) >= 4 and sum(v < -32768 for v in raw) >= 4, raw
    y = rr.resample_at(x, taps, L, M, targets)
    assert 32767 in y and -32768 in y
    if rate:                                                         # designed tables: the gain of the worst input is 1.85 .. 2.14
        g = np.abs(h).sum(axis=1) / 2.0 ** 30
        assert 1.8 < g.min() and g.max() < 2.2, (g.min(), g.max())


def test_rounding_fixture_hits_ties_of_both_signs_and_both_clamps():
    x = rr.all_s16_values()
    assert sorted(set(x.tolist())) == list(range(-32768, 32768))
    idx = range(len(x))
    for name in ("half", "neg_half"):
        acc = rr.accumulate_at(x, rr.ROUNDING_TABLES[name], 1, 1, idx)
        ties = [a for a in acc if a % (1 << 30) == 1 << 29]          # odd multiples of 2^29: exactly half way
        assert sum(a > 0 for a in ties) >= 16384 and sum(a < 0 for a in ties) >= 16384
        # round half up differs from both round-half-away and truncation on the negative ties
        assert all(rr.round_shift(a) == (a >> 30) + 1 for a in ties)
    raw = rr.resample_raw_at(x, rr.ROUNDING_TABLES["sum"], 1, 1, idx)
    assert max(raw) > 32767 and min(raw) < -32768 and 32767 in raw and -32768 in raw and 32768 in raw and -32769 in raw
    # the global-window run (1, 17, 2) of the same values tiled 17 times puts every s16 value under tap 0
    assert sorted(set(np.tile(x, 17)[::17].tolist())) == list(range(-32768, 32768))


@pytest.mark.parametrize("ch", rr.CHANNELS)
def test_downmix_fixture_tells_floor_from_truncation(ch):
    x = rr.downmix_input(ch)
    mono = rr.downmix(x)
    assert mono == ors.downmix(x).tolist()
    sums = [sum(r) for r in x.tolist()]
    assert sums[0] == -32768 * ch and sums[17] == 32767 * ch and mono[0] == -32768 and mono[17] == 32767
    assert [sums[17 * j] for j in (3, 4, 5, 6)] == [-1, -(ch // 2), -(ch // 2) - 1, ch // 2]
    if ch > 1:
        assert [mono[17 * j] for j in (3, 4, 5, 6)] == [0, 0, -1, (ch // 2 * 2) // ch]
        trunc = [int((s + ch // 2) / ch) for s in sums]               # rounding toward zero instead of down
        assert mono[17 * 5] != trunc[17 * 5] and sum(a != b for a, b in zip(mono, trunc)) >= 10
        assert sum(a != s // ch for a, s in zip(mono, sums)) >= 10   # and the C // 2 rounding term matters
    # what the two GPU runs must return: every down-mixed sample, and every 17th
    assert rr.resample_at(x, [[1 << 30, 0]], 1, 1, range(len(x))) == mono
    assert rr.resample_at(x, [[1 << 30, 0]], 1, 17, range(rr.out_len(len(x), 1, 17))) == mono[::17]


def test_lengths_and_sample_sets():
    for (L, M, K), *_ in rr.CASES:
        edges, short = rr.lengths(L, M, K)
        outs = [rr.out_len(n, L, M) for n in edges]
        if L <= M:
            assert outs == [1, 2047, 2048, 2049, 4097], (L, M, K, outs)
        else:                                                        # interpolating: the lengths are the multiples the ratio can reach
            assert outs == [rr.out_len(n, L, M) for n in range(1, len(outs) + 1)] and outs[-2] < 4097 <= outs[-1], (L, M, K, outs)
        assert set(short) == {n for n in (1, 2, K // 2 - 1, K // 2, K, K + 1) if n >= 1}
    idx = rr.sample_indices(10000, 14)
    assert set(range(14)) <= set(idx) and set(range(9986, 10000)) <= set(idx) and {2046, 2047, 2048, 2049, 2050, 4094, 4095, 4096, 4097, 4098} <= set(idx)
    assert rr.sample_indices(3, 8192) == [0, 1, 2]
