"""CPU side of the diarization front end's edge tests (tests/test_diarize_edges_gpu.py): the conditions that the GPU tests' inputs must meet,
checked on the float64 reference alone, and the proof that their bound can fail.

  masked pooling   per edge case (diarize_ref.pool_cases, both 2-byte formats): the yardstick - the deviation of the fp32-in-order restatement
                   from float64 - is positive, every valid row's denominator v1 - v2 / v1 is at least 1, and a ONE-PASS fp32 variance lands
                   beyond FACTOR x the yardstick on every offset case with three or more columns: the GPU bound tells the two apart.
  unmasked pooling the fp32-in-order restatement of resnet_tstp_kernel against resnet_ref.tstp_stats: its yardstick is positive and of the size
                   that fp32 sums of T terms allow.
  masks            the constructed threshold rows (3 against 4 clean columns, 1 against 2 columns, frame count against column count) have
                   exactly the stated column counts in the reference, and diarize.masks_host agrees with the reference on them and on the
                   (F, T4) grid of the GPU test.
  decode           NaN and infinities: the reference's `>` scan and diarize.decode_host.

Each test prints its figures before it asserts; profiles/r23_diarize_edges_parity.txt records them."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diarize_ref as DR  # noqa: E402
from conftest import sub  # noqa: E402

dz = sub("diarize")
FACTOR = 3.0
MASK_F = (1, 2, 63, 64, 65, 589)


def case_id(case):
    sh, data, wk = case
    return "x".join(map(str, sh)) + f"-{data}-{wk}"


# ------------------------------------------------------------------------------------------------ masked pooling
@pytest.mark.parametrize("fmt", [0, 2])
@pytest.mark.parametrize("case", DR.pool_cases(), ids=case_id)
def test_pool_cases_meet_their_conditions_and_reject_one_pass(case, fmt):
    shape, data, wk = case
    x, w, valid, want, yard = DR.pool_reference(shape, data, wk, fmt)
    ok = valid.bool()
    wd = w.double()
    den = (wd.sum(-1) - (wd * wd).sum(-1) / wd.sum(-1))[ok]
    last = x.float().permute(0, 3, 1, 2)
    one = float((DR.weighted_stats_fp32_one_pass(last, w).double() - want)[ok].abs().max())
    print(f"pool case {case_id(case)} fmt={fmt}: valid rows {int(ok.sum())}/{ok.numel()} yardstick {yard:.3e} bound {FACTOR * yard:.3e} "
          f"least denominator {float(den.min()):.4f} one-pass max|d| {one:.3e} = {one / yard:.1f} x yardstick")
    assert torch.isfinite(want[ok]).all() and yard > 0.0
    assert float(den.min()) >= 1.0
    if shape[4] >= 4:                                                    # the valid mix: invalid rows without and with weights
        assert ok.any() and (w[~ok].sum(-1) == 0).any() and (w[~ok].sum(-1) > 0).any()
    if data == "offset" and shape[2] >= 3:
        assert one > FACTOR * yard, "the bound would let a one-pass variance through"


# ------------------------------------------------------------------------------------------------ unmasked pooling
@pytest.mark.parametrize("fmt", [0, 2])
@pytest.mark.parametrize("data", ["signed", "offset"])
@pytest.mark.parametrize("shape", DR.TSTP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tstp_in_order_restatement(shape, data, fmt):
    """An fp32 sum of T terms is off by at most (T - 1) 2^-24 sum |x|, so the mean by T 2^-24 max|x|; the deviation of the std is of the
    same order (the squares are summed about the mean).  The restatement is a restatement only if it stays inside 4 x that."""
    x, want, yard = DR.tstp_reference(shape, data, fmt)
    T = shape[2]
    size = 4 * T * 2.0 ** -24 * float(x.float().abs().max())
    print(f"tstp case {'x'.join(map(str, shape))}-{data} fmt={fmt}: yardstick {yard:.3e} bound {FACTOR * yard:.3e} (fp32 sums allow {size:.3e})")
    assert torch.isfinite(want).all() and 0.0 < yard <= size


# ------------------------------------------------------------------------------------------------ masks
def random_cls(rng, B, F):
    """Class runs of 1 .. min(90, F // 4 + 2) frames, a third of them silence."""
    cls = np.zeros((B, F), np.uint8)
    for b in range(B):
        i = 0
        while i < F:
            n = int(rng.integers(1, min(90, F // 4 + 2) + 1))
            cls[b, i:i + n] = 0 if rng.random() < 0.3 else rng.integers(1, 7)
            i += n
    return cls


def mask_t4s(F):
    return sorted({t for t in (1, F - 1, F, F + 1, 2 * F + 3, 126) if t >= 1})


def constructed_masks(F, T4):
    """Chunks whose speaker 0 sits exactly on a threshold of the masks rule -> (cls [n, F], rows): a row is (name, chunk, active columns,
    clean columns, clean frames, used_clean, valid) of speaker 0, the counts being what the chunk is BUILT to have.  Class 1 is speaker 0
    alone, class 4 speakers 0 and 1.  The columns span both 64-lane sweeps of the kernel where T4 > 64."""
    def frame(j):
        return min(F - 1, (j * F) // T4)
    cols = [0, 20, 63, 64, 100, 125] if T4 > 64 else [0, 17, 30, 41, 55, 63]
    assert len({frame(j) for j in cols}) == 6 and cols[-1] == T4 - 1
    plans = [("3 clean + 2 overlapped", [cols[0], cols[2], cols[3]], [cols[1], cols[5]], 0, 1),
             ("4 clean + 2 overlapped", [cols[0], cols[2], cols[3], cols[4]], [cols[1], cols[5]], 1, 1),
             ("1 clean column", [cols[3]], [], 0, 0),
             ("1 overlapped column", [], [cols[5]], 0, 0),
             ("2 clean columns", [cols[2], cols[3]], [], 0, 1),
             ("1 clean + 1 overlapped", [cols[0]], [cols[4]], 0, 1)]
    cls = np.zeros((len(plans) + 1, F), np.uint8)
    rows = []
    for c, (name, clean, over, used, valid) in enumerate(plans):
        for j in clean:
            cls[c, frame(j)] = 1
        for j in over:
            cls[c, frame(j)] = 4
        rows.append((name, c, len(clean) + len(over), len(clean), len(clean), used, valid))
    # four clean FRAMES on two columns (a column's frame, the two frames behind it that no column takes, the next column's frame) and two
    # overlapped columns: the frame count says 4, the column count 2.  Needs frames that no column takes: F > T4.
    j = 30
    if frame(j + 1) - frame(j) >= 3:
        c = len(plans)
        cls[c, frame(j):frame(j) + 3] = 1
        cls[c, frame(j + 1)] = 1
        cls[c, frame(cols[0])] = cls[c, frame(cols[5])] = 4
        rows.append(("4 clean frames on 2 columns + 2 overlapped", c, 4, 2, 4, 0, 1))
    else:
        cls = cls[:-1]
    return cls, rows


CONSTRUCTED = [(589, 126), (64, 64)]


def check_constructed(F, T4, w, info):
    """The asserts of the constructed rows on a (w, info) pair - the reference's here, the GPU's in the GPU test."""
    cls, rows = constructed_masks(F, T4)
    counts = DR.column_counts(cls, T4)
    for name, c, n_full, n_clean, clean_frames, used, valid in rows:
        assert counts[c, 0].tolist() == [n_full, n_clean], (name, counts[c, 0])          # on the reference first
        assert info[c, 0].tolist() == [n_full + (clean_frames - n_clean), clean_frames, used, valid], (name, info[c, 0])
        assert int(w[c, 0].sum()) == (n_clean if used else n_full), name
    return rows


@pytest.mark.parametrize("F,T4", CONSTRUCTED)
def test_constructed_mask_rows_sit_on_their_thresholds(F, T4):
    cls, _ = constructed_masks(F, T4)
    w, info = DR.masks(cls, T4)
    rows = check_constructed(F, T4, w, info)
    # at F = T4 every frame is a column: the frame count cannot disagree with the column count, and that row is built at F = 589 only
    assert len(rows) == (7 if F > T4 else 6)
    print(f"constructed masks F={F} T4={T4}: " + "; ".join(f"{r[0]} -> columns {r[2]}/{r[3]} clean frames {r[4]} used_clean {r[5]} valid {r[6]}" for r in rows))
    hw, hinfo = dz.masks_host(cls, T4)
    assert np.array_equal(hw, w) and np.array_equal(hinfo, info)


@pytest.mark.parametrize("F", MASK_F)
def test_masks_host_on_the_edge_grid(F):
    rng = np.random.default_rng(F)
    cls = random_cls(rng, 9, F)
    for T4 in mask_t4s(F):
        w, info = DR.masks(cls, T4)
        hw, hinfo = dz.masks_host(cls, T4)
        assert np.array_equal(hw, w) and np.array_equal(hinfo, info), (F, T4)


# ------------------------------------------------------------------------------------------------ decode
def special_logp():
    """-> (logp [1, 8, 7] fp32, the classes the `>` scan gives them)."""
    nan, inf = np.nan, np.inf
    lp = np.array([[nan] * 7,                                            # all NaN: nothing is greater than class 0
                   [nan, 0.5, 2.0, -1.0, 2.0, 0.0, 1.0],                 # NaN in class 0 only: nothing is greater than a NaN
                   [-inf] * 7,
                   [0.0, -1.0, inf, 3.0, 1.0, inf, 2.0],                 # +inf twice: the lower class
                   [0.0, 1.0, nan, 0.5, 3.0, nan, 3.0],                  # NaN elsewhere is never taken; tie of 4 and 6
                   [-inf, -inf, -inf, -5.0, -inf, -inf, -inf],
                   [-inf, nan, nan, nan, nan, nan, nan],                 # -inf against NaN: class 0 stays
                   [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0 + 2.0 ** -23]], np.float32)[None]
    return lp, np.array([[0, 0, 0, 2, 4, 3, 0, 6]], np.uint8)


def test_decode_special_values_on_the_host():
    lp, want = special_logp()
    assert np.array_equal(DR.decode(lp), want)
    assert np.array_equal(dz.decode_host(lp), want)
    rng = np.random.default_rng(1)
    for F in (1, 255, 256, 257):
        logp = rng.standard_normal((1, F, 7)).astype(np.float32)
        assert np.array_equal(dz.decode_host(logp), DR.decode(logp))
