"""The sdk_*_workspace_bytes sizers are host functions: this file calls them without a GPU.  Per sizer: every argument just outside its range
is refused with 0 and a message in sdk_last_error that names it; at the largest arguments the entry point accepts the result is at least
the sum of the arrays the carve function lists (computed here in Python integers: a 32-bit product in the sizer would wrap and fall short);
over a small grid the result never decreases when one argument grows.  Where the source states the layout exactly the check is equality."""
from __future__ import annotations

import itertools

import pytest

from conftest import sub

LIB = sub("_lib")


@pytest.fixture(scope="module")
def lib():
    return LIB.load_library()


def a256(x: int) -> int:
    return (x + 255) & ~255


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


# ---- the layouts, restated from the carve functions ------------------------------------------------------------------------------------
def kmeans_bytes(n, d, k):
    """csrc/kmeans.hip km_carve, every array rounded up to 256 bytes: Ct [d][64] f64, maxcos [n] f64, sval [ceil(n / 256)] f64, srow [ceil(n / 256)]
    i32, psum [ceil(n / 1024)][k][d] f64, pcnt [ceil(n / 1024)][k] i32, done and changed (one i32 each)."""
    nblk, nseg = cdiv(n, 256), cdiv(n, 1024)
    return a256(d * 64 * 8) + a256(n * 8) + a256(nblk * 8) + a256(nblk * 4) + a256(nseg * k * d * 8) + a256(nseg * k * 4) + 2 * a256(4)


def samples_runs_bytes(G):
    """csrc/samples.hip sm_layout, int32 cells: kind, grp_start, grp_end [G] each, grp_solo [G + 1], kept_start [G], four tables of
    ceil(G / 2048) workgroups, counts [4]; the sum rounded up to 256 bytes."""
    return a256(4 * (5 * G + 1 + 4 * cdiv(G, 2048) + 4))


def samples_score_bytes(M, S, d):
    """csrc/samples.hip sdk_samples_score: c [M][d] and msum [S][d] float64, plus 256 bytes, rounded up to 256."""
    return a256((M + S) * d * 8 + 256)


def rows_gram_bytes(n, k):
    """csrc/spectral.hip: partial Gram blocks [ceil(n / 256)][k][k] fp32."""
    return cdiv(n, 256) * k * k * 4


def smooth_bytes(G):
    """csrc/smooth.hip: one int4 and one int2 per packed frame, plus 256 bytes, rounded up to 256 (never 0: that is the refusal)."""
    return a256(G * 24 + 256)


def stream_bytes(R, capacity, d):
    """csrc/stream.hip st_layout, per stream: the header (frontier, reach int64; K and three pads int32; n [64] int32 = 288 bytes), sums and unit
    [capacity][d] float64, nc and cnt [1024] uint16, act [1024][capacity rounded up to 8] uint16; rounded up to 256; R such blocks."""
    return R * a256(288 + 2 * capacity * d * 8 + 2 * 1024 * 2 + 1024 * ((capacity + 7) & ~7) * 2)


def plda_enroll_bytes(P, S):
    """csrc/plda_score.hip pe_layout, int32, every array rounded up to 256 bytes: off [S + 1], cursor [S], rows [max(P, 1)]."""
    return a256((S + 1) * 4) + a256(S * 4) + a256(max(P, 1) * 4)


def vbx_doubles(n, D, S):
    """csrc/vbx.hip vb_carve, float64 cells: rho [n][D], G [n], lse [n], Npart [ceil(n / 64)][S], Fpart [ceil(n / 64)][S][D], lsepart [ceil(n / 64)],
    N [S], alphaT [D][S], cs [S], es [S], prev, done."""
    nblk = cdiv(n, 64)
    return n * D + 2 * n + nblk * S + nblk * S * D + nblk + S + D * S + 2 * S + 2


def vbx_hmm_doubles(n, D, S):
    """sdk_vbx's plus logp, lf, lb [n][S], m [n], pipart [ceil(n / 64)][S], pinew [S]."""
    return vbx_doubles(n, D, S) + 3 * n * S + n + cdiv(n, 64) * S + S


EXACT = {
    "sdk_smooth_turns_workspace_bytes": (smooth_bytes, [(0,), (1,), (326,), ((1 << 30) - 1,)]),
    "sdk_stream_state_bytes": (stream_bytes, [(1, 1, 64), (3, 4, 64), (65, 64, 512), (1 << 20, 64, 512)]),
    "sdk_plda_enroll_workspace_bytes": (plda_enroll_bytes, [(0, 1), (150, 40), (1 << 22, 1 << 20)]),
    "sdk_kmeans_rows_workspace_bytes": (kmeans_bytes, [(1, 64, 1), (1100, 64, 3), (257, 192, 64), (1024, 512, 7), (1025, 512, 7), (65536, 512, 64)]),
    "sdk_samples_runs_workspace_bytes": (samples_runs_bytes, [(1,), (2047,), (2048,), (2049,), (2060,), (1 << 20,), ((1 << 30) - 1,)]),
    "sdk_samples_score_workspace_bytes": (samples_score_bytes, [(0, 0, 64), (1, 0, 64), (21, 9, 64), (21, 9, 512), ((1 << 24) - 1, (1 << 24) - 1, 512)]),
    "sdk_rows_gram_workspace_bytes": (rows_gram_bytes, [(1, 1), (256, 32), (257, 7), (300, 7), (1 << 24, 32)]),
}



# ---- the rest of the layouts that are bounded by design, restated exactly ------------------------------------------------------------------
def matvec_bytes(N):
    """csrc/spectral.hip: X packed per 32-row tile (4 x 64 x 8 bf16 a tile, rounded up to 256), partial Y tiles (MV_MAX_WG = 1024 plus three per
    512-row group, each [512][32] fp32), a part count per group, 256 bytes."""
    return a256(cdiv(N, 32) * 4 * 64 * 8 * 2) + (1024 + 3 * cdiv(N, 512)) * 512 * 32 * 4 + cdiv(N, 512) * 4 + 256


def laplacian_bytes(N, k):
    """csrc/collective.hip lt_layout, every array rounded up to 256: four blocks [N][k] fp32, two vectors [N] fp32, four [32][32] fp32 matrices, a
    256-byte flag, the mat-vec's workspace and the Gram partials."""
    return 4 * a256(N * k * 4) + 2 * a256(N * 4) + 4 * a256(32 * 32 * 4) + 256 + a256(matvec_bytes(N)) + a256(rows_gram_bytes(N, k))


def knn_reverse_bytes(n, P):
    """csrc/nmesc.hip: counts [ceil(n / 256)][n] int32 and a vector [n] int32, each rounded up to 256."""
    return a256(cdiv(n, 256) * n * 4) + a256(n * 4)


def cohort_bytes(N, M, K):
    """csrc/snorm.hip: a score block [rows][M] fp32, rows = min(max(N, 1), the row block): the row block is 64 MiB / (4 M) rounded down to 64,
    at least 64 and at most 1024.  Bounded in N by design: the rows go through in blocks."""
    rb = (64 << 20) // (4 * M)
    rb = min(max(rb - rb % 64, 64), 1024)
    return a256(min(max(N, 1), rb) * M * 4)


def trial_calib_bytes(N, M, max_blocks):
    """csrc/trials.hip: one row of [2][8] float64 partials per workgroup; the grid is min(64 x 64 tiles, 512, max_blocks if > 0): bounded by design."""
    grid = min(cdiv(N, 64) * cdiv(M, 64), 512)
    grid = min(grid, max_blocks) if max_blocks > 0 else grid
    return a256(grid * 16 * 8)


def plda_fit_bytes(n, d, K, scatter):
    """csrc/plda_fit.hip pf_layout, each rounded up to 256: scale [n] f64, colpart [nblk][d] f64, scatpart [nblk][d][d] f64 (with the scatter), off
    [K + 1] int64; nblk = ceil(n / row block), row block = max(512, 64 ceil(n / 16384)): at most 256 blocks, bounded by design."""
    rb = max(512, 64 * cdiv(n, 16384))
    nblk = cdiv(n, rb)
    return a256(n * 8) + a256(nblk * d * 8) + (a256(nblk * d * d * 8) if scatter else 0) + a256((K + 1) * 8)


def plda_score_bytes(N, S, k):
    """csrc/plda_score.hip ps_plan / ps_layout: 64 x 64 tiles; a speaker split is max(4, ceil(column tiles / ceil(1024 / row tiles))) tiles wide;
    with more than one split the lists [nsplit][N][4] float64 then int32, each rounded up to 256; else nothing (256: 0 is the refusal)."""
    ntn, nts = max(cdiv(N, 64), 1), cdiv(S, 64)
    tps = max(cdiv(nts, cdiv(1024, ntn)), 4)
    nsplit = cdiv(nts, tps)
    e = nsplit * N * 4
    return (a256(e * 8) + a256(e * 4)) if nsplit > 1 and N > 0 else 256


EXACT.update({
    "sdk_affinity_matvec_workspace_bytes": (matvec_bytes, [(1,), (600,), (512,), (513,), (1 << 20,), (1 << 24,)]),
    "sdk_laplacian_topk_workspace_bytes": (laplacian_bytes, [(1, 1), (300, 4), (257, 32), (1 << 24, 32)]),
    "sdk_knn_reverse_workspace_bytes": (knn_reverse_bytes, [(2, 1), (65, 64), (300, 64), (65536, 64)]),
    "sdk_cohort_stats_workspace_bytes": (cohort_bytes, [(0, 1, 1), (70, 300, 20), (5000, 300, 20), (5000, 1 << 20, 5), ((1 << 31) - 1, 1 << 20, 1 << 20)]),
    "sdk_trial_calib_workspace_bytes": (trial_calib_bytes, [(1, 1, 0), (130, 70, 0), (130, 70, 3), (5000, 5000, 0), (1 << 20, 1 << 20, 0), (1 << 20, 1 << 20, (1 << 31) - 1)]),
    "sdk_plda_fit_stats_workspace_bytes": (plda_fit_bytes, [(1, 1, 0, 0), (300, 64, 7, 1), (513, 512, 19, 1), (1 << 24, 512, 1 << 24, 1), (1 << 24, 512, 1 << 24, 0)]),
    "sdk_plda_score_workspace_bytes": (plda_score_bytes, [(0, 1, 1), (130, 300, 3), (130, 255, 1), (200, 1100, 4), (65536, 1 << 20, 4), (1, 1 << 20, 4), (4096, 1 << 20, 4)]),
})


@pytest.mark.parametrize("sizer", sorted(EXACT))
def test_sizer_equals_its_layout(lib, sizer):
    layout, shapes = EXACT[sizer]
    for args in shapes:
        assert int(getattr(lib, sizer)(*args)) == layout(*args), (sizer, args)


# ---- lower bounds at the largest accepted arguments ------------------------------------------------------------------------------------
# (sizer, the largest arguments, the least the arrays need there, what they are)
LOWER = [
    ("sdk_vbx_workspace_bytes", (65536, 128, 65536), 8 * vbx_doubles(65536, 128, 65536), "csrc/vbx.hip vb_carve (vbx_doubles above); Fpart alone is 2^36 bytes"),
    ("sdk_vbx_hmm_workspace_bytes", (65536, 128, 65536), 8 * vbx_hmm_doubles(65536, 128, 65536), "vb_carve plus the HMM's arrays (vbx_hmm_doubles above)"),
    ("sdk_knn_reverse_workspace_bytes", (65536, 64), 4 * 65536 * cdiv(65536, 256), "include/sdk_hip.h: 4 n ceil(n / 256) bytes of counts + O(n)"),
    ("sdk_affinity_workspace_bytes", (1 << 20, 1 << 20), (1 << 20) * (2 * 8 * 4 + 8 + 2 * 1024 * 16),
     "csrc/scoring.hip ws_layout: cand_val, cand_idx [N][8], ubound, flag_rows [N], part_s, part_i [N][ceil(P / 1024)][4]"),
    ("sdk_fbank_workspace_bytes", (4096, 160000), 4096 * 1001 * 80 * 4, "fp32 log-mel [B][1 + S / 160][80]"),
    ("sdk_se_workspace_bytes", (65536, 1024, 128), 65536 * (2 * 1024 + 128) * 4, "fp32 [B][C] means, [B][Cse] hidden, [B][C] gates"),
    ("sdk_samples_score_workspace_bytes", ((1 << 24) - 1, (1 << 24) - 1, 512), 2 * ((1 << 24) - 1) * 512 * 8, "c [M][d] and msum [S][d] float64"),
]


# The sizers above that are only lower-bounded, at the smallest, a middle and the largest argument set this file gives them: the values the
# library returned on the commit before every layout moved onto csrc/workspace.hpp's carver (read from that build, not derived), which a
# layout must go on returning byte for byte.
PINNED = {
    "sdk_vbx_workspace_bytes": {(1, 64, 1): 3840, (130, 64, 17): 105984, (65536, 128, 65536): 69393195520},
    "sdk_vbx_hmm_workspace_bytes": {(1, 64, 1): 5376, (130, 64, 17): 161792, (65536, 128, 65536): 173010330112},
    "sdk_affinity_workspace_bytes": {(1, 1): 1792, (600, 1025): 124160, (1 << 20, 1 << 20): 34435236096},
    "sdk_fbank_workspace_bytes": {(1, 400): 960, (7, 16000): 226240, (4096, 160000): 1312030720},
    "sdk_se_workspace_bytes": {(1, 256, 64): 2304, (3, 1024, 128): 26112, (65536, 1024, 128): 570425344},
}
PINNED_PRECISE_ECAPA = {(1, 9): 551424, (3, 230): 37976064, (1 << 20, 2047): 117651502268416}      # ecapa_desc(precision=1) below


@pytest.mark.parametrize("sizer", sorted(PINNED))
def test_lower_bounded_sizers_return_the_pinned_values(lib, sizer):
    for args, want in PINNED[sizer].items():
        assert int(getattr(lib, sizer)(*args)) == want, (sizer, args)


def test_precise_ecapa_sizer_returns_the_pinned_values(lib):
    hp = ecapa_desc(precision=1)
    for (B, T), want in PINNED_PRECISE_ECAPA.items():
        assert int(lib.sdk_ecapa_workspace_bytes(C.byref(hp), B, T)) == want, (B, T)


@pytest.mark.parametrize("sizer,args,least,why", LOWER, ids=[row[0] for row in LOWER])
def test_sizer_covers_its_arrays_at_the_largest_arguments(lib, sizer, args, least, why):
    got = int(getattr(lib, sizer)(*args))
    assert got >= least, f"{sizer}{args} = {got} < {least} ({why}; sdk_last_error: {lib.sdk_last_error()})"


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
# (sizer, accepted arguments, [(position, value just outside, the name the message must hold)])
REFUSED = [
    ("sdk_kmeans_rows_workspace_bytes", (10, 64, 2), [(0, 0, "n="), (0, 65537, "n="), (1, 0, "d="), (1, 96, "d="), (1, 576, "d="), (2, 0, "k="), (2, 65, "k="), (2, 11, "k=")]),
    ("sdk_samples_runs_workspace_bytes", (10,), [(0, -1, "G="), (0, 1 << 30, "G=")]),
    ("sdk_samples_score_workspace_bytes", (4, 2, 64), [(0, -1, "M="), (0, 1 << 24, "M="), (1, -1, "S="), (1, 1 << 24, "S="), (2, 0, "d="), (2, 96, "d="), (2, 576, "d=")]),
    ("sdk_smooth_turns_workspace_bytes", (10,), [(0, -1, "G="), (0, 1 << 30, "G=")]),
    ("sdk_vbx_workspace_bytes", (10, 64, 3), [(0, 0, "n="), (0, 65537, "n="), (1, 96, "D="), (2, 0, "S=")]),
    ("sdk_vbx_hmm_workspace_bytes", (10, 64, 3), [(0, 0, "n="), (0, 65537, "n="), (1, 96, "D="), (2, 0, "S=")]),
    ("sdk_knn_reverse_workspace_bytes", (10, 9), [(0, 1, "n="), (0, 65537, "n="), (1, 8, "P=")]),
    ("sdk_plda_enroll_workspace_bytes", (10, 3), [(0, -1, "P="), (0, (1 << 22) + 1, "P="), (1, 0, "S="), (1, (1 << 20) + 1, "S=")]),
    ("sdk_plda_score_workspace_bytes", (10, 3, 1), [(0, -1, "N="), (0, 65537, "N="), (1, 0, "S="), (1, (1 << 20) + 1, "S="), (2, 0, "k="), (2, 5, "k=")]),
    ("sdk_cohort_stats_workspace_bytes", (10, 20, 5), [(0, -1, "N="), (1, 0, "M="), (1, (1 << 20) + 1, "M="), (2, 0, "K="), (2, 21, "K=")]),
    ("sdk_affinity_workspace_bytes", (5, 7), [(0, 0, "N="), (1, 0, "P=")]),
    ("sdk_affinity_matvec_workspace_bytes", (5,), [(0, 0, "N="), (0, (1 << 24) + 1, "N="), (0, (1 << 31) - 1, "N=")]),
    ("sdk_fbank_workspace_bytes", (2, 16000), [(0, 0, "B="), (1, 0, "S=")]),
    ("sdk_trial_calib_workspace_bytes", (5, 5, 0), [(0, 0, "N="), (0, (1 << 20) + 1, "N="), (1, 0, "M="), (1, (1 << 20) + 1, "M="), (2, -1, "max_blocks=")]),
    ("sdk_rows_gram_workspace_bytes", (5, 4), [(0, 0, "n="), (0, (1 << 24) + 1, "n="), (0, (1 << 31) - 1, "n="), (1, 0, "k="), (1, 33, "k=")]),
    ("sdk_plda_fit_stats_workspace_bytes", (5, 64, 3, 1), [(0, 0, "n="), (0, (1 << 24) + 1, "n="), (1, 0, "d="), (1, 513, "d="), (2, -1, "K="), (2, (1 << 24) + 1, "K=")]),
    ("sdk_laplacian_topk_workspace_bytes", (5, 4), [(0, 0, "N="), (0, (1 << 24) + 1, "N="), (0, (1 << 31) - 1, "N="), (1, 0, "k="), (1, 33, "k=")]),
    ("sdk_se_workspace_bytes", (2, 256, 64), [(0, 0, "B="), (1, 0, "C="), (2, 0, "Cse=")]),
    ("sdk_stream_state_bytes", (3, 4, 64), [(0, 0, "R="), (0, (1 << 20) + 1, "R="), (1, 0, "capacity="), (1, 65, "capacity="), (2, 0, "d="), (2, 96, "d="), (2, 576, "d=")]),
]


@pytest.mark.parametrize("sizer,good,bad", REFUSED, ids=[row[0] for row in REFUSED])
def test_sizer_refuses_each_argument_just_outside_its_range(lib, sizer, good, bad):
    fn = getattr(lib, sizer)
    assert int(fn(*good)) > 0, (sizer, good, lib.sdk_last_error())
    for pos, value, name in bad:
        args = list(good)
        args[pos] = value
        assert int(fn(*good)) > 0                                       # a call that succeeds in between: the message below is this refusal's
        got = int(fn(*args))
        msg = (lib.sdk_last_error() or b"").decode()
        assert got == 0, f"{sizer}{tuple(args)} = {got}: not refused"
        assert sizer in msg and f"{name}{value}" in msg, f"{sizer}{tuple(args)}: sdk_last_error does not name the argument: {msg!r}"


# ---- monotone ---------------------------------------------------------------------------------------------------------------------------
GRID = {
    "sdk_kmeans_rows_workspace_bytes": ([64, 255, 256, 257, 1024, 1025, 3000], [64, 128, 512], [1, 3, 64]),
    "sdk_samples_runs_workspace_bytes": ([0, 1, 2047, 2048, 2049, 5000, 100000],),
    "sdk_samples_score_workspace_bytes": ([0, 1, 21, 1000], [0, 1, 9, 500], [64, 128, 512]),
    "sdk_smooth_turns_workspace_bytes": ([0, 1, 255, 256, 257, 5000, 100000],),
    "sdk_vbx_workspace_bytes": ([1, 63, 64, 65, 130, 2049], [64, 128], [1, 15, 16, 17, 300]),
    "sdk_vbx_hmm_workspace_bytes": ([1, 63, 64, 65, 130, 2049], [64, 128], [1, 15, 16, 17, 300]),
    "sdk_plda_enroll_workspace_bytes": ([0, 1, 150, 5000], [1, 40, 3000]),
    "sdk_plda_score_workspace_bytes": ([0, 1, 63, 64, 65, 130, 5000], [1, 63, 64, 65, 300, 5000], [1, 2, 4]),
    "sdk_cohort_stats_workspace_bytes": ([1, 70, 5000], [40, 300, 5000], [1, 20, 40]),
    "sdk_rows_gram_workspace_bytes": ([1, 255, 256, 257, 1000], [1, 7, 32]),
    "sdk_affinity_workspace_bytes": ([1, 127, 128, 129, 600, 5000], [1, 4, 1024, 1025, 2048, 2049, 40000]),
    "sdk_affinity_matvec_workspace_bytes": ([1, 255, 256, 257, 5000],),
    "sdk_fbank_workspace_bytes": ([1, 2, 7, 64], [400, 16000, 32000, 48000]),
    "sdk_trial_calib_workspace_bytes": ([1, 64, 65, 5000], [1, 64, 65, 5000], [1, 2, 64]),
    "sdk_stream_state_bytes": ([1, 3, 65], [1, 2, 4, 64], [64, 256, 512]),
    "sdk_plda_fit_stats_workspace_bytes": ([1, 300, 5000], [64, 512], [0, 7, 300], [0, 1]),
    "sdk_laplacian_topk_workspace_bytes": ([1, 255, 256, 257, 5000], [1, 7, 32]),
    "sdk_se_workspace_bytes": ([1, 3, 64], [256, 1024], [64, 128]),
}


@pytest.mark.parametrize("sizer", sorted(GRID))
def test_sizer_never_decreases_when_an_argument_grows(lib, sizer):
    fn, axes = getattr(lib, sizer), GRID[sizer]
    value = {args: int(fn(*args)) for args in itertools.product(*axes)}
    assert max(value.values()) > 0, sizer
    for args, v in value.items():
        for pos, axis in enumerate(axes):
            at = axis.index(args[pos])
            if at + 1 < len(axis):
                more = args[:pos] + (axis[at + 1],) + args[pos + 1:]
                assert value[more] >= v, f"{sizer}{more} = {value[more]} < {sizer}{args} = {v}"


def test_knn_reverse_sizer_never_decreases_with_n(lib):
    """P follows n (P = min(64, n - 1)), so the grid is over n alone."""
    ns = [2, 3, 64, 65, 66, 255, 256, 257, 300, 5000, 65536]
    v = [int(lib.sdk_knn_reverse_workspace_bytes(n, min(64, n - 1))) for n in ns]
    assert v[0] > 0 and all(b >= a for a, b in zip(v, v[1:])), list(zip(ns, v))


# ---- the sizers that take a descriptor or host offsets -------------------------------------------------------------------------------------------
import ctypes as C  # noqa: E402

FUSED_MAX = 224          # sdk_asp_fused_max_frames()


def ecapa_desc(C_=1024, Cm=3072, scale=8, Cse=128, A=128, precision=0):
    d = LIB.EcapaDesc()
    d.n_mels_padded, d.channels, d.sub_channels, d.scale, d.se_channels, d.attn_channels, d.mfa_channels = 128, C_, C_ // scale, scale, Cse, A, Cm
    d.embed_dim, d.n_blocks, d.kernel0, d.precision = 192, 3, 5, precision
    return d


def ecapa_bytes(lib, d, B, T, full_logits=False):
    """csrc/sdk_api.hip fwd_layout (precision 0 and 2), each rounded up to 256: X0, U, R, Z [B T][C], Sa, Sb [B T][C / scale], CAT, H [B T][Cm], AH
    [B T][A] 16-bit; ctx [B][2 Cm], ubias [B][A] fp32; the logits [B T][Cm] fp32 only off the fused pooling (T > 224, A != 128, or the masked
    forward: else 256 bytes); pooled [B][2 Cm] fp32; the SE workspace; the GEMM's column statistics; means [B][C] fp32."""
    M, Cc, Cm, S, A = B * T, d.channels, d.mfa_channels, d.sub_channels, d.attn_channels
    fused = not full_logits and A == 128 and T <= FUSED_MAX
    return (4 * a256(M * Cc * 2) + 2 * a256(M * S * 2) + 2 * a256(M * Cm * 2) + a256(M * A * 2) + a256(B * 2 * Cm * 4) + a256(B * A * 4)
            + a256(256 if fused else M * Cm * 4) + a256(B * 2 * Cm * 4) + a256((2 * B * Cc + B * d.se_channels) * 4)
            + a256(int(lib.sdk_conv_gemm_stats_bytes(M, Cm, 2))) + a256(B * Cc * 4))


def ecapa_masked_bytes(lib, d, B, T, S):
    """masked_layout: the forward's layout with the logits, then ctx [B S][2 Cm], ubias [B S][A], pooled [B S][2 Cm] fp32 and ok [B S] int32."""
    R, Cm, A = B * S, d.mfa_channels, d.attn_channels
    return a256(ecapa_bytes(lib, d, B, T, True)) + 2 * a256(R * 2 * Cm * 4) + a256(R * A * 4) + a256(R * 4)


# the largest batch the forwards take: B * T = 2^31 - 2^20 - ... below 2^31 (check_forward_args); every [B T][C] product is past 2^32 there
BIG_B, BIG_T = 1 << 20, 2047
ECAPA_SHAPES = [(1, 9), (2, 50), (2, 201), (2, FUSED_MAX), (2, FUSED_MAX + 1), (3, 230), (BIG_B, BIG_T), (BIG_B * 2047, 1)]


def test_ecapa_sizers_equal_their_layouts(lib):
    assert lib.sdk_asp_fused_max_frames() == FUSED_MAX
    for d in (ecapa_desc(), ecapa_desc(256, 768, 2, 64, 128), ecapa_desc(512, 1536, 8, 128, 64, precision=2)):
        for B, T in ECAPA_SHAPES:
            assert int(lib.sdk_ecapa_workspace_bytes(C.byref(d), B, T)) == ecapa_bytes(lib, d, B, T), (d.channels, B, T)
            for S in (1, 3, 8):
                assert int(lib.sdk_ecapa_masked_workspace_bytes(C.byref(d), B, T, S)) == ecapa_masked_bytes(lib, d, B, T, S), (d.channels, B, T, S)
    # the precise mode keeps every activation as two fp16 planes: at least twice the 16-bit activations of the layout above
    hp, d0 = ecapa_desc(precision=1), ecapa_desc()
    for B, T in ECAPA_SHAPES:
        M = B * T
        assert int(lib.sdk_ecapa_workspace_bytes(C.byref(hp), B, T)) >= 2 * M * (4 * d0.channels + 2 * d0.sub_channels + 2 * d0.mfa_channels + d0.attn_channels) * 2


def xvector_desc(couts=(512, 512, 512, 512, 1536), n_feats=128, precision=0):
    XV = sub("xvector")
    d = XV.XVectorDesc()
    d.n_frame_layers, d.n_feats, d.embed_dim = len(couts), n_feats, 512
    for i, c in enumerate(couts):
        d.cout[i], d.cin[i], d.kernel[i], d.dilation[i] = c, n_feats if i == 0 else couts[i - 1], 1, 1
    d.off[62] = precision
    return d


def xvector_bytes(d, B, T):
    """xv_layout: two activation buffers [B T][the widest layer] of 2 bytes (4 in the precise mode: two fp16 planes) and the statistics
    [B][2 x the last layer] fp32, each rounded up to 256."""
    couts = [d.cout[i] for i in range(d.n_frame_layers)]
    return 2 * a256(B * T * max(couts) * (4 if d.off[62] == 1 else 2)) + a256(B * 2 * couts[-1] * 4)


def test_xvector_sizer_equals_its_layout(lib):
    for precision in (0, 1, 2):
        d = xvector_desc(precision=precision)
        for B, T in [(1, 9), (2, 9), (2, 50), (5, 50), (BIG_B, BIG_T)]:
            assert int(lib.sdk_xvector_workspace_bytes(C.byref(d), B, T)) == xvector_bytes(d, B, T), (precision, B, T)


def resnet_desc(n_feats=80, widths=(32, 64, 128, 256), blocks=(3, 4, 6, 3)):
    RN = sub("resnet")
    d = RN.ResNetDesc()
    d.n_feats, d.embed_dim, d.precision, d.n_layers = n_feats, 256, 0, 4
    for i in range(4):
        d.width[i], d.blocks[i] = widths[i], blocks[i]
    return d


def resnet_bytes(d, B, T, rows=1):
    """rn_layout: three buffers [B][the largest map F x T x C of the stem and the four stages, halved in F and T from the second stage on] of 2
    bytes and the statistics [B rows][2 C4 F4] fp32, each rounded up to 256."""
    F, Tl, big = d.n_feats, T, d.n_feats * T * d.width[0]
    for l in range(4):
        if l:
            F, Tl = (F - 1) // 2 + 1, (Tl - 1) // 2 + 1
        big = max(big, F * Tl * d.width[l])
    return 3 * a256(B * big * 2) + a256(B * rows * 2 * d.width[3] * F * 4)


def test_resnet_sizers_equal_their_layout(lib):
    d = resnet_desc()
    for B, T in [(1, 9), (2, 101), (4, 101), (3, 1000), (BIG_B, BIG_T)]:
        assert int(lib.sdk_resnet_workspace_bytes(C.byref(d), B, T)) == resnet_bytes(d, B, T), (B, T)
        for S in (1, 2, 3, 2047):
            assert int(lib.sdk_resnet_masked_workspace_bytes(C.byref(d), B, T, S)) == resnet_bytes(d, B, T, S), (B, T, S)


def _desc_sizers():
    e, x, r = ecapa_desc(), xvector_desc(), resnet_desc()
    return [("sdk_ecapa_workspace_bytes", e, (2, 50)), ("sdk_ecapa_masked_workspace_bytes", e, (2, 50, 3)), ("sdk_xvector_workspace_bytes", x, (2, 50)),
            ("sdk_resnet_workspace_bytes", r, (2, 101)), ("sdk_resnet_masked_workspace_bytes", r, (2, 101, 2))]


def test_descriptor_sizers_refuse_each_argument_just_outside_its_range(lib):
    names = ("B", "T", "S")
    for sizer, d, good in _desc_sizers():
        fn = getattr(lib, sizer)
        bad = [(i, 0) for i in range(len(good))] + [(0, (1 << 31) // good[1] + 1)]          # B * T reaches 2^31
        if sizer == "sdk_ecapa_masked_workspace_bytes":
            bad.append((2, 9))
        for pos, value in bad:
            args = list(good)
            args[pos] = value
            assert int(fn(C.byref(d), *good)) > 0
            assert int(fn(C.byref(d), *args)) == 0, (sizer, args)
            msg = (lib.sdk_last_error() or b"").decode()
            assert sizer in msg and f"{names[pos]}={value}" in msg, (sizer, args, msg)
        assert int(fn(None, *good)) == 0 and sizer in (lib.sdk_last_error() or b"").decode()
    hp = ecapa_desc(precision=1)                                                            # the masked forward is not built for the precise mode
    assert int(lib.sdk_ecapa_masked_workspace_bytes(C.byref(hp), 2, 50, 3)) == 0 and "precision=1" in lib.sdk_last_error().decode()


def test_descriptor_sizers_never_decrease_when_an_argument_grows(lib):
    grids = {2: ([1, 2, 3, 64], [9, 50, 201, FUSED_MAX, FUSED_MAX + 1, 1000]), 3: ([1, 2, 3, 64], [9, 50, 201, FUSED_MAX, FUSED_MAX + 1, 1000], [1, 2, 3, 8])}
    for sizer, d, good in _desc_sizers():
        fn, axes = getattr(lib, sizer), grids[len(good)]
        value = {args: int(fn(C.byref(d), *args)) for args in itertools.product(*axes)}
        assert min(value.values()) > 0, sizer
        for args, v in value.items():
            for pos, axis in enumerate(axes):
                at = axis.index(args[pos])
                if at + 1 < len(axis):
                    more = args[:pos] + (axis[at + 1],) + args[pos + 1:]
                    assert value[more] >= v, f"{sizer}{more} = {value[more]} < {sizer}{args} = {v}"


def linkage_bytes(bounds):
    """csrc/ahc.hip: a table of one 48-byte record per problem, then per problem of n rows the distances [n][n] float64, a vector [n] float64
    and three [n] int32, every array rounded up to 256."""
    return a256(48 * (len(bounds) - 1)) + sum(a256(n * n * 8) + a256(n * 8) + 3 * a256(n * 4) for n in (b - a for a, b in zip(bounds, bounds[1:])))


LINKAGE = ("sdk_centroid_linkage_workspace_bytes", "sdk_linked_linkage_workspace_bytes")


def _off(bounds):
    a = (C.c_int32 * len(bounds))(*bounds)
    return a, len(bounds) - 1


@pytest.mark.parametrize("sizer", LINKAGE)
def test_linkage_sizers(lib, sizer):
    fn = getattr(lib, sizer)
    # exact, up to the largest problems: 65536 rows each (8 n^2 = 2^35 bytes a problem), as many as int32 offsets hold
    for bounds in ([0, 1], [0, 33, 34, 70], [0, 90, 150], [0, 65536], [0] + [65536 * i for i in range(1, 6)], [0] + [65536 * i for i in range(1, 32768)] + [(1 << 31) - 1]):
        a, G = _off(bounds)
        assert int(fn(a, G, 64)) == linkage_bytes(bounds), (sizer, bounds[:5], G)
    # monotone: a row more in a problem, a problem more, never less
    base = int(fn(*_off([0, 33, 34, 70]), 64))
    assert int(fn(*_off([0, 33, 34, 71]), 64)) >= base and int(fn(*_off([0, 34, 35, 71]), 64)) >= base and int(fn(*_off([0, 33, 34, 70, 71]), 64)) >= base
    assert int(fn(*_off([0, 33, 34, 70]), 2048)) >= base                                    # the width does not enter
    # refusals, each named
    for bounds, G, dim, word in (([0, 5], 0, 64, "G=0"), ([0, 5], 1, 0, "dim=0"), ([0, 5], 1, 2049, "dim=2049"), ([1, 5], 1, 64, "offsets[0]=1"),
                                 ([0, 5, 5], 2, 64, "problem 1"), ([0, 65537], 1, 64, "n=65537")):
        a, _ = _off(bounds)
        assert int(fn(*_off([0, 5]), 64)) > 0
        assert int(fn(a, G, dim)) == 0, (sizer, bounds, G, dim)
        msg = lib.sdk_last_error().decode()
        assert sizer in msg and word in msg, (sizer, bounds, msg)
    assert int(fn(None, 1, 64)) == 0 and "offsets is null" in lib.sdk_last_error().decode()
