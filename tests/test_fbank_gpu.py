"""csrc/fbank.hip against float64 where the 80 dB floor, the 1e-10 guard, the tile edges, the switch between the two normaliser kernels,
the three storage formats and full-scale input engage.  References, inputs and every bound come from tests/fbank_ref.py, whose
preconditions tests/test_fbank_cpu.py checks without a device; no bound here was read off a device.

The tests call sdk_fbank_fmt with a workspace they own and read the fp32 log-mel [B, T, 80] back from it: include/sdk_hip.h documents
`ws` as exactly that ("fp32 log-mel scratch").  A later kernel that fuses the normalisation into the tile kernel and no longer writes
the log-mel there will have to move this read (to a debug output of its own, say); the end-to-end and independence tests below do
not depend on it.

Every numeric assertion prints its worst ratio first; profiles/r17_fbank_parity.txt keeps one run's figures (pytest -s)."""
import numpy as np
import pytest
import torch

import fbank_ref as R
from conftest import sub

check = sub("_lib").check

pytestmark = pytest.mark.gpu

DEFAULT_LDF = {0: 128, 1: 192, 2: 128}
LDFS = {0: (80, 96, 128), 1: (160, 176, 192), 2: (80, 96, 128)}
_runs = {}


def _call(engine, fn, pcm_dev, B, S, precision, ldf, extra=()):
    """One launch into buffers of the test's own: (stored 16-bit patterns [B, T, ldf], fp32 log-mel [B, T, 80]), numpy."""
    T = 1 + S // R.HOP
    wsb = engine.lib.sdk_fbank_workspace_bytes(B, S)
    assert wsb == B * T * R.N_MELS * 4
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device="cuda")                     # NaN patterns: an element left unwritten shows
    feats = torch.full((B * T, ldf), 0x5555, dtype=torch.int16, device="cuda")          # and so does a padding column left unwritten
    check(fn(engine.ctx, pcm_dev.data_ptr(), *extra, B, S, engine.fbank_tables().data_ptr(), feats.data_ptr(), ldf, ws.data_ptr(), wsb, precision,
             torch.cuda.current_stream().cuda_stream), "fbank")
    torch.cuda.synchronize()
    return feats.cpu().numpy().view(np.uint16).reshape(B, T, ldf), ws.view(torch.float32).cpu().numpy().reshape(B, T, R.N_MELS)


def _fbank(engine, pcm: np.ndarray, precision: int, ldf: int = None):
    B, S = pcm.shape
    return _call(engine, engine.lib.sdk_fbank_fmt, torch.from_numpy(np.array(pcm)).cuda(), B, S, precision, ldf or DEFAULT_LDF[precision])


def _case_run(engine, S: int, precision: int):
    """The seven rows of length S at the default ldf: launched once per session and shared (read-only)."""
    key = (S, precision)
    if key not in _runs:
        bits, L = _fbank(engine, R.case(S)[0], precision)
        bits.flags.writeable = False
        L.flags.writeable = False
        _runs[key] = (bits, L)
    return _runs[key]


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("S", R.SHAPES)
def test_raw_logmel_inside_interval(engine, S, precision):
    """The device's fp32 log-mel, before floor and mean, lies inside fbank_ref.raw_interval for all seven rows: the bf16 hi+lo table with
    the hardware log2 (precision 0) and the fp16 hi+lo table with log10f (precision 1).  tests/test_fbank_cpu.py shows that a table
    without its lo plane leaves this interval at every length but S = 1."""
    _, L = _case_run(engine, S, precision)
    lo, hi = R.case_interval(S, precision)
    assert np.isfinite(L).all()
    half, mid = (hi - lo) / 2, (hi + lo) / 2
    ratio = (L.astype(np.float64) - mid) / half
    worst = np.abs(ratio).reshape(len(R.ROWS), -1).max(axis=1)
    # where the interval's lower end sits on the 1e-10 guard a correct result sits on that end too (ratio -1 + the log term): the second
    # figure leaves those elements out
    off_guard = np.where(lo > -99.0, np.abs(ratio), 0.0).reshape(len(R.ROWS), -1).max(axis=1)
    print(f"raw log-mel S={S} T={L.shape[1]} precision {precision}: worst (got - centre) / half-width per row (a)..(g) {worst.round(4).tolist()}, "
          f"off the guard {off_guard.round(4).tolist()}; median half-width {np.median(half):.2e} dB")
    assert worst.max() <= 1.0, f"row ({R.ROWS[int(worst.argmax())]}) leaves the interval: {worst.max():.3f} half-widths"


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("S", R.SHAPES)
def test_normaliser_is_bit_exact(engine, S, precision):
    """feats == norm_fp32(the device's own log-mel) bit for bit, in bf16, fp16 planes and one fp16 plane, at three row strides each.
    T = 480 runs fbank_norm_lds_kernel and T = 481 fbank_norm_kernel; the source's claim that the two are bit-identical is what
    holds both to the same restatement.  Padding columns of every plane are +0; the all-zero row gives all-zero features.
    (That last assertion found the one defect of this file's first run: with the mean taken as a plain sum of T values over T, digital
    silence at T = 33 came out as 2^-17 dB in every element, because 33 copies of 3.0103f * log2(1e-10f) do not sum exactly.  Both
    normalisers now sum differences from the bin's first frame.)"""
    pcm = R.case(S)[0]
    fmt = R.FMT[precision]
    for ldf in LDFS[precision]:
        bits, L = _case_run(engine, S, precision) if ldf == DEFAULT_LDF[precision] else _fbank(engine, pcm, precision, ldf)
        assert np.isfinite(L).all()
        want = R.norm_fp32(L, fmt, ldf)
        diff = bits != want
        print(f"normaliser S={S} T={L.shape[1]} precision {precision} ldf {ldf}: {int(diff.sum())} of {diff.size} stored elements differ from the fp32 restatement")
        assert not diff.any(), f"first difference at (row, frame, column) {tuple(np.argwhere(diff)[0])}"
        h = ldf // 2 if fmt == "planes" else 0
        pad = np.ones(ldf, dtype=bool)
        pad[:R.N_MELS] = False
        pad[h:h + R.N_MELS] = False
        assert not bits[..., pad].any(), "padding columns must be zero"
        assert not bits[2].any(), "all-zero input must give all-zero features"
        assert np.isfinite(R.decode(bits, fmt)).all()


@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("S", R.SHAPES)
def test_end_to_end_with_the_floor_engaged(engine, S, precision):
    """Rows (a), (b) and (e) against oracle.fbank.  Tolerance per element: fbank_ref.feature_interval, i.e. raw_interval carried through
    floor and mean, the normaliser's fp32 bound and half an ulp of the storage format.  Elements that are clamped whatever the error
    (silence under a loud peak) must equal flo - mean to the same bound; they are reported on their own."""
    fmt = R.FMT[precision]
    bits, _ = _case_run(engine, S, precision)
    got = R.decode(bits, fmt)
    want = R.case_features(S)
    lo, hi, sure = R.feature_interval(*R.case_interval(S, precision), fmt)
    assert (lo <= want).all() and (want <= hi).all()
    d = got - want
    ratio = np.where(d >= 0, d / np.maximum(hi - want, 1e-300), -d / np.maximum(want - lo, 1e-300))
    for row in R.FLOOR_ROWS:
        r, s = ratio[row], sure[row]
        print(f"end to end S={S} precision {precision} row ({R.ROWS[row]}): worst |got - oracle| / tolerance {r.max():.4f} (|d| max {np.abs(d[row]).max():.3e} dB); "
              f"{int(s.sum())} elements surely clamped, worst there {r[s].max() if s.any() else 0.0:.4f}")
    assert ratio[list(R.FLOOR_ROWS)].max() <= 1.0


@pytest.mark.parametrize("S", R.SHAPES)
def test_rows_are_independent(engine, S):
    """Row i alone equals row i inside the batch, and permuting the rows permutes the output: bit for bit, log-mel and features."""
    pcm = R.case(S)[0]
    perm = np.array([4, 0, 6, 2, 5, 1, 3])
    for precision in (0, 1, 2):
        bits, L = _case_run(engine, S, precision)
        pb, pL = _fbank(engine, pcm[perm], precision)
        assert np.array_equal(pb, bits[perm]) and np.array_equal(pL.view(np.uint32), L[perm].view(np.uint32))
        for i in range(len(R.ROWS)):
            b1, L1 = _fbank(engine, pcm[i:i + 1], precision)
            assert np.array_equal(b1[0], bits[i]) and np.array_equal(L1[0].view(np.uint32), L[i].view(np.uint32)), f"row ({R.ROWS[i]}) precision {precision}"


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_windows_past_the_end_equal_zero_padded_rows(engine, precision):
    """sdk_fbank_windows_fmt on a recording whose second half is digital silence: windows inside, flush with the end, running past the end and
    starting on the last sample equal sdk_fbank_fmt on the zero-padded rows bit for bit - with the floor engaged in every window."""
    rec = np.concatenate([R.case(5120)[0][1], R.case(5120)[0][0]])               # row (b), then row (a): noise, a gap, a tone, silence
    n = len(rec)
    for S in (4960, 160):
        starts = np.array([0, 3001, n - S, n - S + 1, n - 3 * S // 5, n - 1], dtype=np.int32)       # 4960: 0.6 S before the end still holds some tone
        rows = np.zeros((len(starts), S), dtype=np.int16)
        for i, s0 in enumerate(starts):
            rows[i, :min(S, n - s0)] = rec[s0:s0 + S]
        assert rows[-1, 0] == rec[-1] and not rows[-1, 1:].any()
        want_bits, want_L = _fbank(engine, rows, precision)
        sdev = torch.from_numpy(starts).cuda()
        got_bits, got_L = _call(engine, engine.lib.sdk_fbank_windows_fmt, torch.from_numpy(np.array(rec)).cuda(), len(starts), S, precision, DEFAULT_LDF[precision],
                                extra=(n, sdev.data_ptr()))
        assert np.array_equal(got_L.view(np.uint32), want_L.view(np.uint32))
        assert np.array_equal(got_bits, want_bits)
        clamped = (want_L < want_L.reshape(len(starts), -1).max(axis=1)[:, None, None] - 80.0).reshape(len(starts), -1).mean(axis=1)
        print(f"windows S={S} precision {precision}: share of clamped elements per window {clamped.round(3).tolist()}")
        if S == 4960:
            assert (clamped[[1, 2, 3, 4]] > 0).all(), "the floor must engage in the windows that hold the gap or the silence"


@pytest.mark.parametrize("S", [5120, 76640, 76800])
def test_two_runs_give_the_same_bits(engine, S):
    pcm = R.case(S)[0]
    for precision in (0, 1, 2):
        bits, L = _case_run(engine, S, precision)
        b2, L2 = _fbank(engine, pcm, precision)
        assert np.array_equal(b2, bits) and np.array_equal(L2.view(np.uint32), L.view(np.uint32))
