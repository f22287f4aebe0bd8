"""GPU checks of the diarization front end off its one production shape: the masked and the unmasked statistics pooling of csrc/resnet.hip
(sdk_resnet_masked_pool, sdk_resnet_pool) and the masks, centroid and decode kernels of csrc/diarize.hip, at idle lanes, strided channel
loops, second speaker groups, valid = 0 rows, the LDS limit, both 64-lane sweeps, the 256-pair tile edge and the thresholds of the masks rule.

Pooling bound: the project's convention - the GPU lies within FACTOR = 3 x the deviation of the fp32-in-order restatement
(diarize_ref.weighted_stats_fp32_in_order, diarize_ref.tstp_stats_fp32_in_order) from float64, measured inside the test on the same inputs.
tests/test_diarize_edges_cpu.py shows on the CPU that the yardstick is positive for every case and that a one-pass fp32 variance lands 220 to
39 000 x beyond it on every offset case with three or more columns, so the bound can fail.  The integer kernels are compared bit for bit,
the centroids with the asserts of test_diarize_assign_gpu.test_centroids_against_float64.  Each test prints its figures before it asserts;
those of a run on an MI355X are recorded in profiles/r23_diarize_edges_parity.txt."""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assign_ref as AR  # noqa: E402
import diarize_ref as DR  # noqa: E402
from test_diarize_edges_cpu import (CONSTRUCTED, FACTOR, MASK_F, case_id, check_constructed, constructed_masks, mask_t4s, random_cls,  # noqa: E402
                                    special_logp)

PKG = "speaker-diarization-toolkit_amd"
dz = importlib.import_module(f"{PKG}.diarize")
LIB = importlib.import_module(f"{PKG}._lib")
pytestmark = pytest.mark.gpu


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ 1: masked pooling
def masked_pool(engine, x, w, valid, fmt):
    """x [B, F4, T4, C] 2-byte, w [B, S, T4], valid [B, S] (host) -> [B, S, 2 C F4] fp32 (host); the output starts as NaN."""
    B, F4, T4, Cc = x.shape
    S = w.shape[1]
    xd, wd, vd = x.cuda().contiguous(), w.cuda().contiguous(), valid.cuda().contiguous()
    out = torch.full((B, S, 2 * Cc * F4), float("nan"), dtype=torch.float32, device="cuda")
    LIB.check(engine.lib.sdk_resnet_masked_pool(engine.ctx, xd.data_ptr(), B, F4, T4, Cc, S, wd.data_ptr(), vd.data_ptr(), out.data_ptr(), fmt,
                                                torch.cuda.current_stream().cuda_stream), "sdk_resnet_masked_pool")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("fmt", [0, 2])
@pytest.mark.parametrize("case", DR.pool_cases(), ids=case_id)
def test_masked_pooling_edges(engine, case, fmt):
    shape, data, wk = case
    B, F4, T4, Cc, S = shape
    x, w, valid, want, yard = DR.pool_reference(shape, data, wk, fmt)
    ok = valid.bool()
    wd = w.double()
    den = float((wd.sum(-1) - (wd * wd).sum(-1) / wd.sum(-1))[ok].min())
    got = masked_pool(engine, x, w, valid, fmt)
    err = float((got.double() - want)[ok].abs().max())
    print(f"masked pooling {case_id(case)} fmt={fmt}: valid rows {int(ok.sum())}/{ok.numel()} least denominator {den:.4f} yardstick {yard:.3e} "
          f"bound {FACTOR * yard:.3e} gpu max|d| {err:.3e} = {err / yard:.2f} x yardstick")
    assert yard > 0.0 and den >= 1.0                                     # conditions on the inputs, from the reference alone
    assert np.isfinite(err) and err <= FACTOR * yard
    # rows with valid == 0 are exactly 0.0 in both halves (all-zero weights make 0 / 0 inside the kernel: not NaN either)
    assert (bits(got[~ok]) == 0).all(), "a valid = 0 row is not +0.0 everywhere"
    assert same_bits(got, masked_pool(engine, x, w, valid, fmt)), "two runs differ"
    if B > 1:                                                            # a segment alone equals the segment in the batch
        for b in range(B):
            assert same_bits(got[b:b + 1], masked_pool(engine, x[b:b + 1], w[b:b + 1], valid[b:b + 1], fmt)), f"segment {b} depends on the batch"
    if S > 4:                                                            # a row depends on its own weights only: the S-row call against S = 1
        for b in range(B):
            for s in range(S):
                alone = masked_pool(engine, x[b:b + 1], w[b:b + 1, s:s + 1], valid[b:b + 1, s:s + 1], fmt)
                assert same_bits(got[b, s], alone[0, 0]), f"row {s} of segment {b} depends on the other rows"


# ------------------------------------------------------------------------------------------------ 2: unmasked pooling
def pool(engine, x, fmt):
    B, F4, T4, Cc = x.shape
    xd = x.cuda().contiguous()
    out = torch.full((B, 2 * Cc * F4), float("nan"), dtype=torch.float32, device="cuda")
    LIB.check(engine.lib.sdk_resnet_pool(engine.ctx, xd.data_ptr(), B, F4, T4, Cc, out.data_ptr(), fmt, torch.cuda.current_stream().cuda_stream),
              "sdk_resnet_pool")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("fmt", [0, 2])
@pytest.mark.parametrize("data", ["signed", "offset"])
@pytest.mark.parametrize("shape", DR.TSTP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_unmasked_pooling_edges(engine, shape, data, fmt):
    x, want, yard = DR.tstp_reference(shape, data, fmt)
    got = pool(engine, x, fmt)
    err = float((got.double() - want).abs().max())
    print(f"unmasked pooling {'x'.join(map(str, shape))}-{data} fmt={fmt}: yardstick {yard:.3e} bound {FACTOR * yard:.3e} gpu max|d| {err:.3e} "
          f"= {err / yard:.2f} x yardstick")
    assert yard > 0.0
    assert np.isfinite(err) and err <= FACTOR * yard
    assert same_bits(got, pool(engine, x, fmt)), "two runs differ"
    for b in range(shape[0] if shape[0] > 1 else 0):
        assert same_bits(got[b:b + 1], pool(engine, x[b:b + 1], fmt)), f"segment {b} depends on the batch"


def test_unmasked_pooling_refusals(engine):
    x = torch.ones((1, 2, 1, 64), dtype=torch.bfloat16, device="cuda")
    out = torch.full((1, 256), -7.0, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(LIB.SdkError, match="the last map has 1 frames; the unbiased variance needs >= 2"):
        LIB.check(engine.lib.sdk_resnet_pool(engine.ctx, x.data_ptr(), 1, 2, 1, 64, out.data_ptr(), 0, st), "sdk_resnet_pool")
    with pytest.raises(LIB.SdkError, match="sdk_resnet_pool: fmt=1"):
        LIB.check(engine.lib.sdk_resnet_pool(engine.ctx, x.data_ptr(), 1, 1, 2, 64, out.data_ptr(), 1, st), "sdk_resnet_pool")
    torch.cuda.synchronize()
    assert (out == -7.0).all(), "a refused call wrote its output"
    assert torch.isfinite(pool(engine, x.cpu().reshape(1, 1, 2, 64), 0)).all()          # the device is fine after the refusals


# ------------------------------------------------------------------------------------------------ 3: masks
def gpu_masks(engine, cls, T4):
    w, info = dz.diarize_masks(engine, torch.from_numpy(cls).cuda(), T4)
    torch.cuda.synchronize()
    return w.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize("F", MASK_F)
def test_masks_edge_grid_bit_for_bit(engine, F):
    """F below, on and above the 64 lanes; T4 = 1, F - 1, F, F + 1, 2 F + 3 (a frame feeding several columns) and 126; B = 1 and 9."""
    rng = np.random.default_rng(F)
    cls9 = random_cls(rng, 9, F)
    for T4 in mask_t4s(F):
        for cls in (cls9[4:5], cls9):
            w, info = gpu_masks(engine, cls, T4)
            rw, rinfo = DR.masks(cls, T4)
            assert w.shape == rw.shape and np.array_equal(w.view(np.int32), rw.view(np.int32)), (F, T4, len(cls))
            assert np.array_equal(info, rinfo), (F, T4, len(cls))


@pytest.mark.parametrize("F,T4", CONSTRUCTED)
def test_masks_thresholds_bit_for_bit(engine, F, T4):
    cls, _ = constructed_masks(F, T4)
    rw, rinfo = DR.masks(cls, T4)
    check_constructed(F, T4, rw, rinfo)                                  # the reference has exactly the stated counts
    w, info = gpu_masks(engine, cls, T4)
    rows = check_constructed(F, T4, w, info)
    assert np.array_equal(w, rw) and np.array_equal(info, rinfo)
    print(f"masks thresholds F={F} T4={T4}: " + "; ".join(f"{r[0]}: used_clean {info[r[1], 0, 2]} valid {info[r[1], 0, 3]}" for r in rows))


def test_masks_of_no_chunk_are_empty(engine):
    w, info = dz.diarize_masks(engine, torch.empty((0, 589), dtype=torch.uint8, device="cuda"), 126)
    torch.cuda.synchronize()
    assert w.shape == (0, 3, 126) and info.shape == (0, 3, 4)


# ------------------------------------------------------------------------------------------------ 4: centroids
def centroid_case(n, K, d):
    """E [n + 17, d] fp32 unit rows, n of them (ascending, the others hold NaN) training rows with labels in no order."""
    rng = np.random.default_rng([n, K, d])
    R = n + 17
    rows = np.sort(rng.choice(R, n, replace=False)).astype(np.int32)
    E = np.full((R, d), np.nan, np.float32)
    v = rng.standard_normal((n, d)) + 0.5
    E[rows] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    return E, rows, rng.integers(0, K, n).astype(np.int32)


def centroid_ref(E, rows, labels, K):
    """assign_ref.centroids per cluster (its rows added in order in float64, divided by the count, then by the norm); no row: a zero row."""
    out = np.zeros((K, E.shape[1]))
    for k in range(K):
        mine = rows[labels == k]
        if len(mine):
            out[k] = AR.centroids(E, None, mine, np.zeros(len(mine), np.int32))[0]
    return out


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 513])
@pytest.mark.parametrize("K", [1, 7])
@pytest.mark.parametrize("d", [64, 320, 512])
def test_centroids_edges_against_float64(engine, d, K, n):
    """d = 64: three waves add zeros to the norm; d = 320, 512: the second column of a thread is live; n on, below and above the 256-pair
    tile and two tiles plus one.  The bounds are those of test_centroids_against_float64."""
    E, rows, labels = centroid_case(n, K, d)
    ref = centroid_ref(E, rows, labels, K)
    Ed, rd, ld = torch.from_numpy(E).cuda(), torch.from_numpy(rows).cuda(), torch.from_numpy(labels).cuda()
    cent, cent64 = dz.diarize_centroids(engine, Ed, rd, ld, K)
    torch.cuda.synchronize()
    c32, c64 = cent.cpu().numpy(), cent64.cpu().numpy()
    e64 = float(np.abs(c64 - ref).max())
    bound64 = (d + 4) * 2.0 ** -53
    ulps = np.abs(c32.astype(np.float64) - ref.astype(np.float32).astype(np.float64)) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    empty = [k for k in range(K) if not (labels == k).any()]
    print(f"centroids d={d} K={K} n={n}: empty clusters {len(empty)}; cent64 max|d| {e64:.3e} (bound {bound64:.3e}); cent vs fp32(reference): "
          f"worst {ulps.max():.1f} ulp")
    assert np.isfinite(c64).all() and e64 <= bound64 and ulps.max() <= 1.0
    assert np.array_equal(c32, c64.astype(np.float32))
    assert not c64[empty].any() and not c32[empty].any()
    if n == 0:
        assert len(empty) == K and not c64.any() and not c32.any()
    # a cluster without rows gives a zero row; a second run is bit-identical
    cent2, cent64b = dz.diarize_centroids(engine, Ed, rd, ld, K + 1)
    torch.cuda.synchronize()
    assert not cent2[K].any() and not cent64b[K].any() and torch.equal(cent64b[:K], cent64) and torch.equal(cent2[:K], cent)


# ------------------------------------------------------------------------------------------------ 5: powerset decode
def gpu_decode(engine, logp):
    cls = dz.powerset_decode(engine, torch.from_numpy(logp).cuda())
    torch.cuda.synchronize()
    return cls.cpu().numpy()


@pytest.mark.parametrize("F", [1, 255, 256, 257])
def test_decode_block_edges_bit_for_bit(engine, F):
    """C F = 1, one below, on and one above the 256-thread block; the special frames sit wherever the length has room for them."""
    rng = np.random.default_rng(F)
    logp = rng.standard_normal((1, F, 7)).astype(np.float32)
    sp, _ = special_logp()
    if F >= sp.shape[1]:
        logp[0, F - sp.shape[1]:] = sp[0]
    assert np.array_equal(gpu_decode(engine, logp), DR.decode(logp))


def test_decode_special_values(engine):
    """All NaN -> class 0; NaN in class 0 only -> class 0 (nothing is greater than a NaN); all -inf -> class 0; +inf twice -> the lower
    class; NaN elsewhere is never taken."""
    lp, want = special_logp()
    assert np.array_equal(DR.decode(lp), want)
    got = gpu_decode(engine, lp)
    print(f"decode special frames: gpu {got[0].tolist()} reference {want[0].tolist()}")
    assert np.array_equal(got, want)
