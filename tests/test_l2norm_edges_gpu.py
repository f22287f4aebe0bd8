"""sdk_l2norm (csrc/pool_se.hip: l2norm_kernel, one wave per row, four rows per block) off its one shape, against float64 numpy.

E is judged by n 2^-24 |e| with n counted from the kernel: ceil(d / 64) terms per lane, the 6 butterfly steps of the wave sum, then the
square root, the reciprocal and the product - n = ceil(d / 64) + 9.  The library is built without fast-math flags, and hipcc rounds fp32
division and square root correctly by default (csrc/Makefile passes nothing that relaxes them), so each of the last three counts once and no
ulp allowance is added.  (The true first-order error is about half of n: the square root halves the relative error of the sum.)

Eb must be the round-to-nearest-even bf16 of the RETURNED E, bit for bit.  resid is compared with the float64 norm of the returned E - Eb by
the same n (the differences are exact in fp32; their squares, the two sums and the square root round), and separately from below: the
affinity rescore guard relies on resid not being an underestimate.

What the kernel does outside unit-scale rows is pinned as include/sdk_hip.h now states it: a squared norm that overflows fp32 gives a ZERO
row (1 / inf = 0), not the unit row float64 would give; a squared norm that underflows is divided by the 1e-12 floor, as oracle/ecapa.py
does.  No caller produces such rows (embeddings are O(1) .. O(100) per entry), so the behaviour is documented and pinned, not changed."""
import numpy as np
import pytest
import torch

from conftest import sub

pytestmark = pytest.mark.gpu

L = sub("_lib")
EPS32 = 2.0 ** -24
SENT = -7.75
PAD = 2                              # sentinel rows past N in every output


def _s():
    return torch.cuda.current_stream().cuda_stream


def n_ops(d):
    return -(-d // 64) + 6 + 3


def _l2(eng, X, want_e=True, want_eb=True, want_r=True):
    """sdk_l2norm called directly into sentinel-filled outputs with PAD extra rows; returns numpy (E fp32, Eb as fp32, Eb bits, resid fp32),
    None where the output was not asked for; asserts that the rows past N are untouched"""
    N, d = X.shape
    Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda()
    E = torch.full((N + PAD, d), SENT, dtype=torch.float32, device="cuda")
    Eb = torch.full((N + PAD, d), SENT, dtype=torch.bfloat16, device="cuda")
    r = torch.full((N + PAD,), SENT, dtype=torch.float32, device="cuda")
    L.check(eng.lib.sdk_l2norm(eng.ctx, Xd.data_ptr(), N, d, E.data_ptr() if want_e else None, Eb.data_ptr() if want_eb else None,
                               r.data_ptr() if want_r else None, _s()), "sdk_l2norm")
    torch.cuda.synchronize()
    for buf, asked in ((E, want_e), (Eb, want_eb), (r, want_r)):
        assert (buf[N if asked else 0:].float() == SENT).all(), "store past the N rows, or into an output that was not asked for"
    return (E[:N].cpu().numpy() if want_e else None, Eb[:N].float().cpu().numpy() if want_eb else None,
            Eb[:N].cpu().view(torch.int16).numpy() if want_eb else None, r[:N].cpu().numpy() if want_r else None)


def _bf16_bits(E):
    """round-to-nearest-even bf16 of fp32 values, as bit patterns"""
    return torch.from_numpy(E).to(torch.bfloat16).view(torch.int16).numpy()


def _check_rows(X, E, Ebf, Ebits, r, what, judge_resid=True):
    """the full contract on finite rows whose squared norm neither overflows nor underflows"""
    d = X.shape[1]
    n = n_ops(d)
    x = X.astype(np.float64)
    want = x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), 1e-12)
    err, bnd = np.abs(E.astype(np.float64) - want), n * EPS32 * np.abs(want)
    ratio_e = float((err / np.maximum(bnd, 1e-300)).max())
    assert (err <= bnd).all(), f"{what}: E outside n 2^-24 |e| (n = {n}), worst err / bound {ratio_e:.3g}"
    assert np.array_equal(Ebits, _bf16_bits(E)), f"{what}: Eb is not the RNE bf16 of the returned E"
    ratio_r = 0.0
    if judge_resid:
        true = np.sqrt(((E.astype(np.float64) - Ebf.astype(np.float64)) ** 2).sum(1))
        rerr = np.abs(r.astype(np.float64) - true)
        ratio_r = float((rerr / np.maximum(n * EPS32 * true, 1e-300)).max()) if (true > 0).any() else 0.0
        assert (rerr <= n * EPS32 * true).all(), f"{what}: resid outside n 2^-24 ||E - Eb|| (n = {n}), worst err / bound {ratio_r:.3g}"
        assert (r.astype(np.float64) >= true * (1 - n * EPS32)).all(), f"{what}: resid underestimates ||E - Eb||"
    print(f"{what}: E worst err / bound {ratio_e:.3f}, resid worst err / bound {ratio_r:.3f}")


def _rows(N, d, seed):
    """Gaussian rows whose magnitudes span 1e-3 .. 1e3 within the batch (both ends present from N = 2 on)"""
    rng = np.random.default_rng([N, d, seed])
    mag = 10.0 ** rng.uniform(-3, 3, N)
    mag[0], mag[-1] = (1e-3, 1e3) if N > 1 else (1.0, 1.0)
    return (rng.standard_normal((N, d)) * mag[:, None]).astype(np.float32)


@pytest.mark.parametrize("d", [1, 63, 64, 65, 192, 256, 512, 1000])
def test_l2norm_shapes(engine, d):
    """d below, on and off the 64 lanes, the other families' widths; N on the 4-row block edges"""
    for N in (1, 3, 4, 5, 1001):
        X = _rows(N, d, 0)
        assert (np.abs(X).max(1) > 0).all()
        _check_rows(X, *_l2(engine, X), f"l2norm N {N} d {d}")


def _exact_batch(d):
    rng = np.random.default_rng(d)
    singles = [(0, 2.0), (d - 1, -0.5), (min(64, d - 1), 3.0), (min(63, d - 1), 2.0 ** 60), (d // 2, -(2.0 ** -30)), (d // 3, -7.0)]      # all above the 1e-12 floor
    for _, v in singles:                                              # x * fl(1 / |x|) is exactly 1 in fp32 for the values chosen here
        assert np.float32(abs(v)) * (np.float32(1) / np.float32(abs(v))) == np.float32(1)
    X = np.zeros((len(singles) + 7, d), dtype=np.float32)
    for i, (c, v) in enumerate(singles):
        X[i, c] = v
    k = len(singles)
    sign = np.where(np.arange(d) % 2 == 0, 1.0, -1.0)
    X[k + 1] = 1e-30                                                  # squared norm underflows to 0: the 1e-12 floor
    X[k + 2] = 1e18 * sign                                            # d = 192: squared norm 1.9e38, just inside fp32
    X[k + 3] = rng.standard_normal(d) * 1e17
    X[k + 4] = 1e20 * sign                                            # every square overflows
    X[k + 5] = 2e18 * sign                                            # d = 192: squares are finite (4e36), their sum (7.7e38) is not
    X[k + 6] = rng.standard_normal(d)
    return X, k


def test_l2norm_exact_floor_and_overflow_rows(engine):
    d = 192
    X, k = _exact_batch(d)
    E, Ebf, Ebits, r = _l2(engine, X)
    assert np.isfinite(E).all() and np.isfinite(Ebf).all() and np.isfinite(r).all()
    for i in range(k):                                                # one non-zero entry: E = +-1 exactly, Eb = +-1, resid = 0
        want = np.sign(X[i])
        assert np.array_equal(E[i], want) and np.array_equal(Ebf[i], want) and r[i] == 0, (i, E[i][X[i] != 0], r[i])
    assert not E[k].any() and not Ebf[k].any() and r[k] == 0          # the zero row
    # the 1e-12 floor: E = x / 1e-12 as the oracle gives it, within the bound (the fp32 constant, the reciprocal and the product round);
    # resid of a row of norm 1e-17 is the sum of squares near 1e-42, below fp32's normal range: finite, not judged
    _check_rows(X[k + 1:k + 2], E[k + 1:k + 2], Ebf[k + 1:k + 2], Ebits[k + 1:k + 2], r[k + 1:k + 2], "l2norm 1e-30 row", judge_resid=False)
    assert np.abs(E[k + 1].astype(np.float64) - 1e-18).max() <= n_ops(d) * EPS32 * 1e-18 and 0 <= r[k + 1] < 1e-18
    rows = [k + 2, k + 3, k + 6]                                      # up to 1e18 per entry: unit rows within the bound
    _check_rows(X[rows], E[rows], Ebf[rows], Ebits[rows], r[rows], "l2norm rows up to 1e18 per entry")
    assert np.abs(np.sqrt((E[rows].astype(np.float64) ** 2).sum(1)) - 1).max() < 1e-6
    # overflow, pinned as include/sdk_hip.h states it: a squared norm past fp32 gives a zero row (float64 would give a unit row)
    for i in (k + 4, k + 5):
        with np.errstate(over="ignore"):
            assert np.sum(X[i] * X[i], dtype=np.float32) == np.inf
        assert not E[i].any() and not Ebf[i].any() and r[i] == 0, i


@pytest.mark.parametrize("N,d", [(5, 65), (1001, 192), (3, 1000)])
def test_l2norm_null_outputs(engine, N, d):
    """each output is optional: the ones asked for are bit-identical to the all-outputs run, nothing else is written"""
    X = _rows(N, d, 1)
    E, _, Ebits, r = _l2(engine, X)
    for we, wb, wr in ((True, False, False), (False, True, False), (True, True, False), (False, False, True), (False, True, True)):
        E2, _, Eb2, r2 = _l2(engine, X, we, wb, wr)
        assert not we or np.array_equal(E2.view(np.int32), E.view(np.int32)), (we, wb, wr)
        assert not wb or np.array_equal(Eb2, Ebits), (we, wb, wr)
        assert not wr or np.array_equal(r2.view(np.int32), r.view(np.int32)), (we, wb, wr)


@pytest.mark.parametrize("d", [65, 192])
def test_l2norm_nan_stays_in_its_row(engine, d):
    N, bad = 9, 5
    X = _rows(N, d, 2)
    E, _, Ebits, r = _l2(engine, X)
    Xn = X.copy()
    Xn[bad, d - 2] = np.nan
    En, _, Ebn, rn = _l2(engine, Xn)
    keep = np.arange(N) != bad
    assert np.isnan(En[bad]).all() and np.isnan(rn[bad])
    assert np.array_equal(En[keep].view(np.int32), E[keep].view(np.int32)) and np.array_equal(Ebn[keep], Ebits[keep])
    assert np.array_equal(rn[keep].view(np.int32), r[keep].view(np.int32))
    assert np.array_equal(E.view(np.int32), _l2(engine, X)[0].view(np.int32))          # and two calls agree bit for bit
