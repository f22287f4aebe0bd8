"""What tests/test_fbank_gpu.py relies on, checked without a device: that the inputs of tests/fbank_ref.py make the 80 dB floor and the
1e-10 guard engage (and that the control row does not), that raw_interval is wide enough for the oracle's own model of the kernel's
table and too narrow for a table without its lo plane, and that norm_fp32 computes the oracle's normalisation and tells the
wrong-order normalisers apart.  Run with -s for the figures."""
import numpy as np
import pytest

import fbank_ref as R
from oracle import fbank as ofbank

A, B_, C, D, E, F, G = range(7)
TILED = [S for S in R.SHAPES if S >= 4960]          # lengths with at least one full tile of frames


def _shares(S):
    pcm, L = R.case(S)
    n = len(R.ROWS)
    peak = L.reshape(n, -1).max(axis=1)[:, None, None]
    under = (L < peak - ofbank.TOP_DB).reshape(n, -1).mean(axis=1)
    guard = (R.mel_power64(pcm) <= ofbank.AMIN).reshape(n, -1).mean(axis=1)
    return pcm, under, guard


@pytest.mark.parametrize("S", R.SHAPES)
def test_inputs_are_seeded_and_shaped(S):
    pcm = R.inputs(S)
    assert pcm.dtype == np.int16 and pcm.shape == (len(R.ROWS), S)
    assert np.array_equal(pcm, R.inputs(S)), "two calls must give the same bytes"
    assert not pcm[C].any()
    assert set(np.unique(pcm[D])) <= {-32768, 32767}
    if S >= 2:
        assert pcm[D].min() == -32768 and pcm[D].max() == 32767, "row (d) must hold both full-scale levels"
    assert ofbank.num_frames(S) == 1 + S // 160


@pytest.mark.parametrize("S", TILED)
def test_floor_and_guard_engage(S):
    pcm, under, guard = _shares(S)
    print(f"S={S}: share under peak - 80 per row {under.round(3).tolist()}, share at the 1e-10 guard {guard.round(3).tolist()}")
    assert under[A] >= 0.2 and under[E] >= 0.2
    if S <= 5120:                                      # ~2000 zeroed samples are a fifth of the frames only at the short lengths
        assert under[B_] >= 0.2
    assert under[B_] > 0 and guard[A] > 0 and guard[B_] > 0 and guard[C] == 1.0
    assert under[G] == 0 and guard[G] == 0, "row (g) is the control: neither floor nor guard"
    z = int(np.flatnonzero(pcm[B_] == 0)[0])
    assert z % R.HOP != 0, "the zeroed stretch of row (b) must not start on a frame boundary"


@pytest.mark.parametrize("S", R.SHAPES)
def test_interval_holds_the_16_bit_table_and_not_the_8_bit_one(S):
    """oracle.fbank's model of the bf16 hi+lo table (16 significand bits) lies inside raw_interval everywhere; with the lo plane missing
    (8 bits) it leaves it at every length that has a frame with signal off the first sample."""
    pcm, L = R.case(S)
    for precision in (0, 1):
        lo, hi = R.case_interval(S, precision)
        assert (lo <= L).all() and (L <= hi).all(), "the interval must contain the exact value"
        half, mid = (hi - lo) / 2, (hi + lo) / 2
        r16 = np.abs(R.raw_logmel64(pcm, 16) - mid) / half
        r8 = np.abs(R.raw_logmel64(pcm, 8) - mid) / half
        print(f"S={S} precision {precision}: 16-bit table worst ratio {r16.max():.4f}; 8-bit table worst {r8.max():.2f}, "
              f"{int((r8 > 1).sum())} of {r8.size} elements outside; median half-width {np.median(half):.2e} dB")
        assert r16.max() <= 1.0
        if S > 1:
            assert (r8 > 1).any(), "a table without its lo plane stays inside the interval: the bound has no teeth"


@pytest.mark.parametrize("S", R.SHAPES)
def test_norm_fp32_is_the_oracle_normalisation(S):
    pcm, L = R.case(S)
    T = L.shape[1]
    L32 = L.astype(np.float32)
    got = R.norm_values_fp32(L32)
    want = R.case_features(S)
    bound = R.norm_bound(T, L)
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"S={S} T={T}: |norm_fp32 - oracle| worst {err:.3e} = {err / bound:.3f} of the bound {bound:.3e}")
    # + one fp32 rounding of the oracle's own float32 result
    assert err <= bound + R.U32 * np.abs(want).max()
    assert not got[C].any(), "all-zero input: all-zero features"
    for fmt, ldf in (("bf16", 80), ("bf16", 128), ("fp16", 96), ("planes", 160), ("planes", 176), ("planes", 192)):
        bits = R.norm_fp32(L32, fmt, ldf)
        assert bits.shape == (len(R.ROWS), T, ldf) and bits.dtype == np.uint16
        ulp = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "planes": 2.0 ** -22}[fmt]              # half an ulp, relative
        assert (np.abs(R.decode(bits, fmt) - got) <= ulp * np.abs(got) + 2.0 ** -25).all()
        pad = np.ones(ldf, dtype=bool)
        h = ldf // 2 if fmt == "planes" else 0
        pad[:R.N_MELS] = False
        pad[h:h + R.N_MELS] = False
        assert not bits[..., pad].any()


@pytest.mark.parametrize("S", TILED)
def test_norm_fp32_tells_wrong_orders_apart(S):
    """A normaliser that took the mean before the clamp, or the peak per 32-frame tile, differs from norm_fp32 on rows (a) and (b) by far more
    than the fp32 bound within which norm_fp32 equals the oracle."""
    _, L = R.case(S)
    T = L.shape[1]
    L32 = L.astype(np.float32)
    want = R.norm_values_fp32(L32).astype(np.float64)
    bound = R.norm_bound(T, L)
    mean_first = R.norm_values_fp32(L32, clamp_in_mean=False).astype(np.float64)
    per_tile = R.norm_values_fp32(L32, peak_of=R.peak_per_tile).astype(np.float64)
    seen = 0
    for row in (A, B_):
        d1 = np.abs(mean_first[row] - want[row]).max()
        d2 = np.abs(per_tile[row] - want[row]).max()
        # the per-tile peak is the segment's peak in the tile that holds it: the mutant can only show in another tile that has clamped elements
        clamped_tiles = set((np.flatnonzero((L[row] < L[row].max() - 80.0).any(axis=1)) // R.FT).tolist())
        shows = bool(clamped_tiles - {int(np.argmax(L[row].max(axis=1))) // R.FT})
        print(f"S={S} row ({R.ROWS[row]}): mean before clamp differs by {d1:.3f} dB, peak per tile by {d2:.3f} dB "
              f"(clamped elements outside the peak's tile: {shows}); bound {bound:.2e}")
        assert d1 > bound
        if shows:
            assert d2 > bound
            seen += 1
    if T > R.FT:
        assert seen >= 1, "no row at this length can tell a per-tile peak from the segment's"
    if T >= R.NORM_LDS_MAX_T:
        assert seen == 2


@pytest.mark.parametrize("S", TILED)
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_feature_interval_contains_the_oracle(S, fmt):
    pcm, L = R.case(S)
    lo, hi, sure = R.feature_interval(*R.case_interval(S, 0), fmt)
    want = R.case_features(S)
    assert (lo <= want).all() and (want <= hi).all()
    n = sure.reshape(len(R.ROWS), -1).sum(axis=1)
    print(f"S={S} {fmt}: elements clamped whatever the error, per row {n.tolist()}; median width {np.median(hi - lo):.3e} dB")
    assert n[A] > 0 and n[B_] > 0


@pytest.mark.parametrize("T", sorted({1 + S // R.HOP for S in R.SHAPES} | {3, 7, 201}))
def test_norm_fp32_gives_zero_for_a_constant_segment(T):
    """Digital silence on the device is not -100 but 3.0103f * log2(1e-10f), whose multiples are not exact in fp32: three chains of T / 3
    such values, added and divided by T, came out one ulp off the value at T = 33 on the device (features of 2^-17 dB instead of 0).  The
    normaliser sums differences from the first frame, so a constant bin gives +0 whatever its value."""
    v = np.float32(3.0102999566398120) * np.float32(np.log2(np.float32(1e-10)))
    vals = [v, np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(-200)), np.float32(-100.0), np.float32(-33.333332), np.float32(17.1)]
    L32 = np.stack([np.full((T, R.N_MELS), x, dtype=np.float32) for x in vals])
    assert not R.norm_values_fp32(L32).view(np.uint32).any()
