"""Exact reference of the 256^2 GEMM's fused per-segment column statistics (csrc/conv_gemm.hip: tile_stats, the half-tile tail's zero slot,
colstats_finish_kernel), the geometry classes a shape exercises, and the shape table its CPU and GPU tests share.

    C[m, n]   = stored(scale[n] * relu(bias[n] + sum_j sum_c A[seg(m) T + reflect(t(m) + (j - taps // 2) dil), c] * W[n, j Cin + c]) + shift[n])
    mean[b, n] = s / T,   std[b, n] = sqrt(max(q / T - mean^2, 1e-12)),      s = sum of C over the T rows of segment b,  q = sum of C^2

Four things live here:

  * reference(): the float64 convolution on small-integer operands.  Every stored value is then a multiple of one power of two (the common
    quantum, 0.5 with the scales the tests use) that bf16 / fp16 hold unchanged - asserted - and s and q are exact integers of that quantum:
    the reference has no rounding anywhere, so a row credited to the wrong segment, a row counted twice or a slot never written changes it.
  * exact_conditions(): max over segments and columns of sum |v| / quantum and of sum v^2 / quantum^2 is below 2^24.  Every fp32 partial
    sum of the values (or of their squares), in ANY order and any grouping into waves, halves and tiles, is then an integer fp32 holds
    exactly - the kernel's s and q must equal the reference's whatever its reduction tree is.
  * geometry(): the classes of the statistics epilogue a shape (M, T) reaches, written from the layout alone: output rows are cut into
    256-row tiles, each tile into two 128-row halves (the UPPER half holds tile rows 0-127, the LOWER half 128-255), each half into four
    32-row waves, each wave into two 16-row slabs; segment b owns rows [b T, (b + 1) T).  The last tile runs past the matrix when
    M % 256 != 0: its rows >= M do not exist.
        ("nseg", k)              a tile whose rows inside the matrix belong to k = 1, 2 or 3 segments
        ("boundary", o)          a segment boundary strictly inside a wave, o = 1 ... 31 rows after the wave's first row
        ("wave_start", w)        a segment boundary on the first row of wave w = 1, 2 or 3 of its half (w = 0 is a half start: not a class)
        ("edge", kind, half)     the matrix edge inside a wave: kind "lt16" / "eq16" / "gt16" by the wave's rows inside the matrix (the 16-row
                                 slab split), half "upper" / "lower"
        ("outside", half)        a wave of the last tile wholly below the matrix
    A wave cannot hold both a boundary and the matrix edge: M is a multiple of T, so the last boundary inside the matrix is T >= 128 rows
    above the edge and a wave has 32 rows.  geometry() asserts it.
  * SHAPES / operands(): the (T, B) table and the seeded integer operands the CPU and the GPU tests share.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

from oracle import ecapa as oecapa

TILE, HALF, WAVE, SLAB = 256, 128, 32, 16
CIN = 64
VAR_FLOOR = 1e-12                     # var_floor() of csrc/common.hpp
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}

# (T, B): M = T * B.  The last two rows are the shapes tests/test_gpu_kernels.py::test_conv_gemm_fused_column_stats has always used.
SHAPES = [(129, 34), (160, 5), (128, 3), (255, 3), (256, 2), (257, 3), (144, 3), (176, 3), (150, 5), (137, 2), (201, 10), (1500, 2)]

ALL_CLASSES = frozenset(
    [("nseg", k) for k in (1, 2, 3)] + [("boundary", o) for o in range(1, WAVE)] + [("wave_start", w) for w in (1, 2, 3)] +
    [("edge", kind, half) for kind in ("lt16", "eq16", "gt16") for half in ("upper", "lower")] + [("outside", half) for half in ("upper", "lower")])

Ref = namedtuple("Ref", "out quantum s q mean std T")


def reference(A, Wt, Cin, taps, dil, T, bias, scale, shift, relu, fmt):
    """A [M, >= Cin], Wt [N, taps * Cin], bias / scale / shift [N] or None -> Ref(out float64 [M, N], quantum, s, q, mean, std [B, N] float64).
    Asserts that `out` survives the round trip through `fmt` unchanged and that s and q are exact."""
    A = A.double()[:, :Cin]
    M, N = A.shape[0], Wt.shape[0]
    assert M % T == 0
    B = M // T
    t = torch.arange(T)
    out = torch.zeros(M, N, dtype=torch.float64)
    Ab = A.reshape(B, T, Cin)
    for j in range(taps):
        src = oecapa.reflect_index(t + (j - taps // 2) * dil, T)
        out += Ab[:, src, :].reshape(M, Cin) @ Wt.double()[:, j * Cin:(j + 1) * Cin].T
    if bias is not None:
        out += bias.double()
    if relu:
        out.clamp_(min=0.0)
    if scale is not None:
        out = out * scale.double() + shift.double()
    assert torch.equal(out.to(DTYPES[fmt]).double(), out), f"the reference output is not exact in {fmt}"
    quantum = 1.0
    while not torch.equal(torch.round(out / quantum), out / quantum):
        quantum /= 2.0
        assert quantum >= 2.0 ** -20, "no common quantum"
    z = (out / quantum).reshape(B, T, N)
    s_k = z.sum(1)
    q_k = torch.einsum("btn,btn->bn", z, z)
    assert float(z.abs().sum(1).max()) < 2.0 ** 52 and float(q_k.max()) < 2.0 ** 52          # float64 sums of integers: exact
    s, q = s_k * quantum, q_k * quantum * quantum
    var = (q_k * T - s_k * s_k) * (quantum * quantum / (T * T))                               # integers below 2^53: no cancellation error
    assert float((q_k * T).max()) < 2.0 ** 53 and float((s_k * s_k).max()) < 2.0 ** 53
    return Ref(out, quantum, s, q, s / T, var.clamp_min(0.0).sqrt(), T)


def exact_conditions(ref):
    """(max sum |v| / quantum, max sum v^2 / quantum^2, both below 2^24)"""
    B = ref.out.shape[0] // ref.T
    z = (ref.out / ref.quantum).reshape(B, ref.T, -1)
    a, q = float(z.abs().sum(1).max()), float(torch.einsum("btn,btn->bn", z, z).max())
    return a, q, a < 2.0 ** 24 and q < 2.0 ** 24


def geometry(M, T):
    """the set of classes (module docstring) that an M x N output with segments of T rows exercises"""
    assert T >= HALF and M % T == 0 and M >= TILE
    cls = set()
    boundaries = set(range(T, M, T))                       # first rows of segments 1 ... B - 1 (row M is the matrix edge, not a boundary)
    for m0 in range(0, M, TILE):
        rows = range(m0, min(m0 + TILE, M))
        cls.add(("nseg", rows[-1] // T - rows[0] // T + 1))
        for w0 in range(m0, m0 + TILE, WAVE):
            half = "upper" if (w0 - m0) < HALF else "lower"
            inside = [b for b in boundaries if w0 < b < w0 + WAVE]
            edge = w0 < M < w0 + WAVE
            assert len(inside) <= 1 and not (inside and edge), (M, T, w0)
            if inside:
                cls.add(("boundary", inside[0] - w0))
            if w0 in boundaries and (w0 - m0) % HALF:
                cls.add(("wave_start", (w0 - m0) % HALF // WAVE))
            if edge:
                n = M - w0
                cls.add(("edge", "lt16" if n < SLAB else "eq16" if n == SLAB else "gt16", half))
            if w0 >= M:
                cls.add(("outside", half))
    return cls


@lru_cache(maxsize=None)
def operands(T, B, N, taps=1, seed=0):
    """Seeded integer operands: A in [-2, 2], W in [-1, 1], integer bias and shift, scale in {0.5, 1, 2}; every 64th column has zero weights,
    a negative bias and no shift, so that it is all zero after the ReLU.  -> dict of float32 CPU tensors (treat as read-only)."""
    g = torch.Generator().manual_seed(1000 * T + B + 7 * N + taps + seed)
    M = T * B
    A = torch.randint(-2, 3, (M, CIN), generator=g).float()
    Wt = torch.randint(-1, 2, (N, taps * CIN), generator=g).float()
    bias = torch.randint(-3, 4, (N,), generator=g).float()
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (N,), generator=g)]
    shift = torch.randint(-2, 3, (N,), generator=g).float()
    zero = torch.arange(0, N, 64)
    Wt[zero] = 0.0
    bias[zero] = -1.0
    shift[zero] = 0.0
    return dict(A=A, Wt=Wt, bias=bias, scale=scale, shift=shift, zero=zero, M=M, T=T, N=N, taps=taps)


@lru_cache(maxsize=3)
def _case(T, B, N, taps, dil, fmt, seed):
    o = operands(T, B, N, taps, seed)
    return o, reference(o["A"], o["Wt"], CIN, taps, dil, T, o["bias"], o["scale"], o["shift"], True, fmt)


def case(T, B, N, taps=1, dil=1, fmt="bf16", seed=0):
    """(operands, Ref) of a table shape, computed once and shared (treat as read-only)"""
    return _case(T, B, N, taps, dil, fmt, seed)


def expected_mean(ref):
    """the finish kernel's two IEEE operations on the exact s: float32(s) * (float32(1) / float32(T)), in numpy float32"""
    s32 = ref.s.numpy().astype(np.float32)
    assert np.array_equal(s32.astype(np.float64), ref.s.numpy())
    return s32 * (np.float32(1.0) / np.float32(ref.T))


def std_bound(ref):
    """|sd_gpu - sd_exact| allowed per element [B, N] (float64), for columns of exact variance > 0.

    q and s are exact, so the kernel's q * invT - mean^2 is at most three fp32 roundings (two products and the difference, or fewer under any
    FMA contraction) of quantities no larger than m = max(q / T, mean^2): an absolute error of 3 * 2^-24 * m in the variance, i.e. of at
    most 3 * 2^-24 * m / sd in its square root (sqrt(v + e) - sqrt(v) <= e / sqrt(v), a factor 2 more than the first-order term), plus
    the one rounding of the square root itself, 2^-24 * sd.  Doubled for the roundings invT and mean already carry.  Nothing measured."""
    m = torch.maximum(ref.q / ref.T, ref.mean * ref.mean)
    return 2.0 * (3.0 * 2.0 ** -24 * m / ref.std + 2.0 ** -24 * ref.std)
