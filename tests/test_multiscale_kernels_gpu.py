"""GPU checks, exact, of the fused neighbour lists of the multi-scale affinity (sdk_knn_rows_fused, csrc/nmesc.hip; ops_cluster.knn_rows_fused)
against their numpy restatement cluster.knn_rows_fused_host: idx equal, the fused values equal as int64 bit patterns.

Nothing here has a tolerance: per scale the cosine is knn_rows' float64 chain of exact products in column order on both sides, and the sum
over the scales is one rounded product and one rounded addition per scale, in scale order, on both sides."""
from __future__ import annotations

import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_nmesc_kernels_gpu import dev, random_rows, tie_rows  # noqa: E402

PKG = "speaker-diarization-toolkit_amd"
cluster = importlib.import_module(f"{PKG}.cluster")
OC = importlib.import_module(f"{PKG}.ops_cluster")
ops_util = importlib.import_module(f"{PKG}.ops_util")
pytestmark = pytest.mark.gpu

# n: P = n - 1 = 1; the workgroup of 32 query rows (and with it the wave's 8); the 64-candidate tile; 65: P = 64 = n - 1; 97: P = 64 < n - 1,
# two candidate tiles and four workgroups, the last of one row
SIZES = [2, 31, 32, 33, 63, 64, 65, 97]
WIDTHS = [64, 128, 192]                # one, two, three column tiles
SCALES = [1, 2, 3, 8]
MAPS = ["identity", "blocks3", "one_row", "reversed", "unreferenced"]
WEIGHTS = ["equal", "graded", "one_zero"]
ROWS = ["random", "ties"]


def make_maps(kind: str, n: int, S: int):
    """-> (n_all, maps int32 [S, n], the rows of E_all no map names)."""
    if kind == "one_row":                                             # every base row onto ONE row per scale: every c_s is equal, the tie rule orders
        return S, np.repeat(np.arange(S, dtype=np.int32)[:, None], n, axis=1), []
    rows, off, unnamed = [], 0, []
    for s in range(S):
        if kind == "blocks3" and s < S - 1:                           # the usual hop ratio; the base scale stays the identity
            rows.append(off + np.arange(n) // 3)
            off += (n + 2) // 3
        elif kind == "reversed":
            rows.append(off + np.arange(n)[::-1])
            off += n
        else:
            rows.append(off + np.arange(n))
            off += n
        if kind == "unreferenced" and s == 0:                         # one row between the first scale's rows and the rest
            unnamed.append(off)
            off += 1
    return off, np.stack(rows).astype(np.int32), unnamed


def make_weights(kind: str, S: int) -> np.ndarray:
    if kind == "graded":
        w = np.asarray([0.5, 0.3, 0.2]) if S == 3 else np.arange(S, 0, -1, dtype=np.float64) / (S * (S + 1) / 2)
    else:
        w = np.full(S, 1.0 / S)
        if kind == "one_zero" and S > 1:
            w[S // 2] = 0.0
    return w


def make_rows(kind: str, n_all: int, d: int, seed: int):
    return random_rows(n_all, d, seed) if kind == "random" or n_all < 3 else tie_rows(n_all, d, seed)


def assert_fused_equal(engine, E_all, maps, w):
    idx_h, f_h = cluster.knn_rows_fused_host(E_all, maps, w)
    idx, f = OC.knn_rows_fused(engine, dev(E_all), dev(maps), w)
    assert idx.dtype == torch.int32 and f.dtype == torch.float64 and tuple(idx.shape) == idx_h.shape == tuple(f.shape)
    assert np.array_equal(idx.cpu().numpy(), idx_h), (maps.shape, E_all.shape)
    assert np.array_equal(f.cpu().numpy().view(np.int64), f_h.view(np.int64)), (maps.shape, E_all.shape)
    return idx_h, f_h


@pytest.mark.parametrize("n", SIZES)
def test_every_size_width_scale_count_and_map(engine, n):
    """Per n: every width x every scale count x every map, the weights and the rows' kind cycling through their values."""
    t = 0
    for d in WIDTHS:
        for S in SCALES:
            for kind in MAPS:
                n_all, maps, _ = make_maps(kind, n, S)
                E_all = make_rows(ROWS[t % 2], n_all, d, 1000 * n + t)
                idx_h, _ = assert_fused_equal(engine, E_all, maps, make_weights(WEIGHTS[t % 3], S))
                if kind == "one_row":                                 # all values tie: the lower j first
                    assert np.array_equal(idx_h[n - 1], np.arange(min(64, n - 1)))
                t += 1


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("weights", WEIGHTS)
def test_every_weight_on_every_map_and_kind_of_rows(engine, weights, rows):
    """n = 65 (P = 64 = n - 1: every row lists every other, so every fused value is compared), three scales, (0.5, 0.3, 0.2) among them."""
    for t, kind in enumerate(MAPS):
        n_all, maps, _ = make_maps(kind, 65, 3)
        _, f_h = assert_fused_equal(engine, make_rows(rows, n_all, 64, 7 + t), maps, make_weights(weights, 3))
        if rows == "ties" and kind != "one_row":
            assert (np.diff(f_h, axis=1) == 0).any()                  # the input does tie


def test_one_scale_with_the_identity_map_is_knn_rows(engine):
    for n, d in ((33, 64), (97, 192)):
        E = dev(tie_rows(n, d, n, distinct=9))
        idx, cos = OC.knn_rows(engine, E)
        fidx, f = OC.knn_rows_fused(engine, E, dev(np.arange(n, dtype=np.int32)[None, :]), [1.0])
        assert torch.equal(fidx, idx) and torch.equal(f.view(torch.int64), cos.view(torch.int64))


def test_two_runs_give_identical_bytes(engine):
    n_all, maps, _ = make_maps("blocks3", 700, 3)
    E, m = dev(tie_rows(n_all, 128, 3, distinct=40)), dev(maps)

    def run():
        return [t.cpu().numpy().tobytes() for t in OC.knn_rows_fused(engine, E, m, (0.5, 0.3, 0.2))]
    assert run() == run()


def test_nan_rows_count_only_where_a_map_names_them(engine):
    n, d = 70, 64
    n_all, maps, unnamed = make_maps("unreferenced", n, 2)
    clean = random_rows(n_all, d, 11)
    w = [0.5, 0.5]
    ghost = clean.copy()
    ghost[unnamed[0]] = np.nan                                        # a NaN row no map names: not looked at, status 0
    assert_fused_equal(engine, ghost, maps, w)
    n_all3, maps3, _ = make_maps("blocks3", 80, 2)                    # coarse rows 0 .. 26, then 80 base rows: 73 finite candidates > P
    bad = random_rows(n_all3, d, 12)
    bad[[5, 17]] = np.nan                                             # coarse rows: base rows 15 .. 17 and 51 .. 53 name them
    with pytest.raises(ValueError, match="row 5 of E_all") as info:
        OC.knn_rows_fused(engine, dev(bad), dev(maps3), w)
    assert info.value.status == (2, 5)
    idx_h, f_h = cluster.knn_rows_fused_host(bad, maps3, w)           # written all the same: a NaN value is -inf and ranks last
    assert np.array_equal(info.value.idx.cpu().numpy(), idx_h)
    assert np.array_equal(info.value.cos.cpu().numpy().view(np.int64), f_h.view(np.int64))
    assert np.isneginf(f_h[15]).all() and not np.isin(idx_h[0], [15, 16, 17, 51, 52, 53]).any()
    assert_fused_equal(engine, clean, maps, w)                        # the next problem is not affected


def test_map_entries_outside_e_all_raise(engine):
    n_all, maps, _ = make_maps("identity", 40, 2)
    E = dev(random_rows(n_all, 64, 5))
    for entry in (n_all, -1):
        wrong = maps.copy()
        wrong[1, 9] = entry
        wrong[0, 30] = entry
        with pytest.raises(ValueError, match=r"base row 9 has a map entry outside \[0, 80\) \(2 such"):
            OC.knn_rows_fused(engine, E, dev(wrong), [0.5, 0.5])
    idx_h, _ = cluster.knn_rows_fused_host(E.cpu().numpy(), maps, [0.5, 0.5])
    assert np.array_equal(OC.knn_rows_fused(engine, E, dev(maps), [0.5, 0.5])[0].cpu().numpy(), idx_h)


def test_the_wrapper_checks_its_arguments(engine):
    n_all, maps, _ = make_maps("identity", 10, 2)
    E, m = dev(random_rows(n_all, 64, 0)), dev(maps)
    with pytest.raises(ValueError, match="knn_rows_fused: maps must be a contiguous int32 device tensor"):
        OC.knn_rows_fused(engine, E, m.long(), [0.5, 0.5])
    with pytest.raises(ValueError, match="knn_rows_fused: maps must be a contiguous int32 device tensor"):
        OC.knn_rows_fused(engine, E, m.cpu(), [0.5, 0.5])
    with pytest.raises(ValueError, match="knn_rows_fused: E_all must be"):
        OC.knn_rows_fused(engine, E.double(), m, [0.5, 0.5])
    with pytest.raises(ValueError, match="d=96 not supported"):
        OC.knn_rows_fused(engine, torch.zeros((20, 96), device="cuda"), m, [0.5, 0.5])
    with pytest.raises(ValueError, match="S in 1..8"):
        OC.knn_rows_fused(engine, E, torch.zeros((9, 10), dtype=torch.int32, device="cuda"), [1.0] * 9)
    with pytest.raises(ValueError, match="n=1 rows"):
        OC.knn_rows_fused(engine, E, m[:, :1].contiguous(), [0.5, 0.5])
    for bad in ([1.0], [0.5, -0.5], [0.0, 0.0], [float("nan"), 1.0]):
        with pytest.raises(ValueError, match="knn_rows_fused: weights"):
            OC.knn_rows_fused(engine, E, m, bad)


POISON = 0x5A


def test_the_library_refuses_bad_shapes_and_writes_nothing(engine):
    """S = 0, S = 9, d = 96, n = 1 and a P that is not min(64, n - 1), past the wrapper: non-zero, the value named in sdk_last_error(), nothing
    launched - the outputs keep their poison."""
    n, d, S = 10, 64, 2
    E = torch.zeros((64, 128), dtype=torch.float32, device="cuda")
    maps = torch.zeros((9, n), dtype=torch.int32, device="cuda")
    w = (C.c_double * 9)(*([1.0 / 9] * 9))
    out = [torch.full((n * 9 * s,), POISON, dtype=torch.uint8, device="cuda") for s in (4, 8)] + [torch.full((16,), POISON, dtype=torch.uint8, device="cuda")]
    lib = engine.lib

    def call(n_all, d, S, n, P):
        return lib.sdk_knn_rows_fused(engine.ctx, E.data_ptr(), n_all, d, maps.data_ptr(), C.addressof(w), S, n, P, out[0].data_ptr(), out[1].data_ptr(),
                                      out[2].data_ptr(), ops_util._stream())
    for args, named in (((20, d, 0, n, 9), "S=0"), ((20, d, 9, n, 9), "S=9"), ((20, 96, S, n, 9), "d=96"), ((20, d, S, 1, 1), "n=1"),
                        ((20, d, S, n, 8), "P=8"), ((0, d, S, n, 9), "n_all=0")):
        assert call(*args) != 0
        assert named in lib.sdk_last_error().decode() and "sdk_knn_rows_fused" in lib.sdk_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool((t == POISON).all()) for t in out)
    assert call(20, d, S, n, 9) == 0                                  # the same buffers with a good shape: served
    torch.cuda.synchronize()
    assert not bool((out[2] == POISON).all())
