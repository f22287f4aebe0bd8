"""Plain numpy references for sdk_rows_fc (csrc/pool_se.hip) and the case table its CPU and GPU tests share.

    out[b, j] = act(bias[j] + sum_c (in[b, c] * in_scale[c] + in_shift[c]) * wt[c, j])        act 0 none, 1 relu, 2 sigmoid

Three things live here:

  * exact(): the result in int64 arithmetic, for operands that are small integers.  Every kernel adds fp32 products in some fixed order;
    while sum|terms| + |bias| stays below 2^24 every partial sum is an integer fp32 holds exactly, so ANY order gives the int64 result
    bit for bit - and with no operand equal to zero a dropped, duplicated or misplaced term changes it.
  * f64(): the float64 result on the stored fp32 operands, for real data.
  * bound(): the fp32 error bound in the project's form n 2^-24 sum|terms| (tests/test_ecapa_sweeps.py):
        act 0, 1   (Cin + 3) 2^-24 (sum_c |x'_c w_cj| + |bias_j|)                      Cin products and additions, the slice sum, the bias
                   + 2 2^-24 sum_c (|x_c s_c| + |t_c|) |w_cj|   when the affine is given  x' = x s + t rounded once or twice
                   (relu is 1-Lipschitz: the same bound)
        act 2      the above / 4 (sigmoid' <= 1/4)  +  (|v| + 8) 2^-24                   v the float64 pre-activation
    The last term is the error of 1 / (1 + __expf(-v)).  It is NOT a new measurement: it is the figure tests/sweeps_ref.py (se_ref, d_g)
    already carries for the SE gate's sigmoid - the same expression in the same file - and is used unchanged, with no further margin.  It
    is an absolute error on a value in (0, 1): |v| 2^-24 for the rounding of the exponent's argument (relative error of exp = absolute
    error of its argument) and 8 2^-24 for the exponential, the addition and the reciprocal.  tests/test_rows_fc_paths_gpu.py measures the
    sigmoid in isolation in every act = 2 case (float64 on the kernel's own fp32 pre-activation, rows scaled to pre-activations near +-20
    included), prints err / figure and asserts it <= 1.  Measured on an MI355X over the 24 cases (all four kernels, |v| up to 24): worst
    0.151 of the figure, i.e. 0.151 (|v| + 8) 2^-24 - a margin of 6.6x, above the 4x asked of a measured figure.

path() restates the dispatch rule of sdk_rows_fc_path; INT_CASES is the table of (shape, alignment) -> path.
"""
from collections import namedtuple

import numpy as np

EPS32 = 2.0 ** -24
AFF_MAX_BYTES = 64 * 1024            # dynamic LDS of the matrix-pipe kernels: an input affine [2][Cin] fp32, so Cin <= 8192

PLAIN, MFMA4, MFMA16, MFMA16_WLDS = 0, 1, 2, 3
RING_DEPTH = {MFMA4: 4, MFMA16: 4, MFMA16_WLDS: 8}
K_SLICES = {MFMA4: 4, MFMA16: 16, MFMA16_WLDS: 16}


def path(in_addr, ldin, has_affine, wt_addr, Cin, Nout):
    """the kernel sdk_rows_fc launches, from the rule as include/sdk_hip.h states it"""
    mfma_ok = ldin % 4 == 0 and in_addr % 16 == 0 and (not has_affine or Cin * 8 <= AFF_MAX_BYTES)
    if not mfma_ok:
        return PLAIN
    if Cin % 128 == 0 and Cin >= 2048:
        return MFMA16_WLDS if Nout % 32 == 0 and wt_addr % 16 == 0 else MFMA16
    return MFMA4 if Cin % 32 == 0 else PLAIN


def ring(p, Cin):
    """(groups of 8 k per wave, full turns of the register ring, tail groups) of a matrix-pipe path"""
    ng = Cin // K_SLICES[p] // 8
    return ng, ng // RING_DEPTH[p], ng % RING_DEPTH[p]


# One row of the table: the path with the input affine and without it, the shape, and how the operands are laid out:
#   ""  x [B, Cin] and wt contiguous and 16-byte aligned      "ldin+1"  ldin = Cin + 1
#   "wt+4"  wt starts 4 bytes into its buffer                "in+4"    in starts 4 bytes into its buffer
Case = namedtuple("Case", "path_aff path_noaff Cin Nouts layout")
VARIANTS = [("affine+bias", True, True), ("no affine", False, True), ("no bias", True, False)]
B_MFMA, B_PLAIN = (1, 31, 32, 33, 65), (1, 3, 4, 5, 9)          # the 32-row and the 4-row block edges
B_MAX = 65

INT_CASES = (
    [Case(3, 3, c, (32, 192), "") for c in (2048, 2176, 2944, 5120, 6144, 8192)]       # ng 16 (no tail), 17 (tail 1), 23 (tail 7), 40, 48, 64
    + [Case(2, 2, c, (40, 70), "") for c in (2048, 2176, 2432)]                        # ng 16, 17 (tail 1), 19 (tail 3)
    + [Case(2, 2, 2176, (64,), "wt+4")]
    + [Case(1, 1, c, (32, 40, 200), "") for c in (32, 96, 128, 160, 224, 1024, 2016, 2080)]   # ng 1, 3, 4, 5, 7, 32, 63, 65
    + [Case(0, 0, c, (1, 31, 33, 70), "") for c in (1, 33, 511, 513, 1000, 3000)]
    # 512 = the plain kernel's chunk: a multiple of 32, so only a layout the matrix-pipe kernels refuse puts it on the plain kernel
    + [Case(0, 0, 512, (1, 31, 33, 70), "ldin+1")]
    # 8320 = 65 * 128: past the affine's LDS limit with the affine (plain kernel); without it the 16-slice kernel, ng 65 (tail 1)
    + [Case(0, 2, 8320, (1, 31, 33, 70), "")]
    + [Case(0, 0, 128, (64,), "ldin+1"), Case(0, 0, 128, (64,), "in+4")]
)
# one case per path with ldin = Cin + 8 and ldout = Nout + 24 (path, Cin, Nout): all on a ring tail
STRIDED_CASES = [(3, 2944, 192), (2, 2432, 70), (1, 224, 200), (0, 1000, 33)]
# real operands: one steady-state and one tail shape per path (path, Cin, Nout)
REAL_CASES = [(3, 2048, 192), (3, 2944, 32), (2, 2048, 70), (2, 2432, 40), (1, 1024, 200), (1, 224, 40), (0, 512 + 1, 33), (0, 3000, 70)]


def case_id(c):
    return c if isinstance(c, str) else f"p{c.path_aff}{c.path_noaff}-Cin{c.Cin}{'-' + c.layout if c.layout else ''}"


def case_layout(c, Nout):
    """(offset of `in` in bytes, ldin, offset of `wt` in bytes) of a table row"""
    return (4 if c.layout == "in+4" else 0), c.Cin + (1 if c.layout == "ldin+1" else 0), (4 if c.layout == "wt+4" else 0)


def _signed(rng, lo, hi, shape):
    return (rng.integers(lo, hi + 1, shape) * rng.choice([-1, 1], shape)).astype(np.float32)


def int_operands(Cin, Nout, B=B_MAX):
    """x in +-{1..4}, w in +-{1..4}, s in {+-1, +-2}, t in {+-16}, bias in +-{1..1024}: x s + t is never 0 and |x' w| <= 96"""
    rng = np.random.default_rng([Cin, Nout, B])
    x = _signed(rng, 1, 4, (B, Cin))
    w = _signed(rng, 1, 4, (Cin, Nout))
    s = _signed(rng, 1, 2, Cin)
    t = (16 * rng.choice([-1, 1], Cin)).astype(np.float32)
    bias = _signed(rng, 1, 1024, Nout)
    return x, s, t, w, bias


def real_operands(Cin, Nout, B, act, seed=0):
    """x ~ N(0, 1), w ~ N(0, 1) / sqrt(Cin), s in [0.5, 1.5], t ~ N(0, 0.1), bias ~ N(0, 1).  For act = 2 the first four rows are scaled so
    that their largest pre-activation (with the affine) sits near +-20, where the sigmoid's absolute error is asked the most."""
    rng = np.random.default_rng([Cin, Nout, B, act, seed])
    x = rng.standard_normal((B, Cin)).astype(np.float32)
    w = (rng.standard_normal((Cin, Nout)) / np.sqrt(Cin)).astype(np.float32)
    s = rng.uniform(0.5, 1.5, Cin).astype(np.float32)
    t = (0.1 * rng.standard_normal(Cin)).astype(np.float32)
    bias = rng.standard_normal(Nout).astype(np.float32)
    if act == 2:
        for r in range(min(4, B)):
            for _ in range(3):                                       # x' is affine in x, not linear: a few fixed-point steps
                v = np.abs(f64(x[r:r + 1], s, t, w, bias, 0)).max()
                x[r] = (x[r].astype(np.float64) * 20.0 / v).astype(np.float32)
    return x, s, t, w, bias


def exact(x, s, t, w, bias, act):
    """int64 result for integer operands (act 0 or 1); s, t and bias may be None"""
    assert act in (0, 1)
    xi = x.astype(np.int64)
    if s is not None:
        xi = xi * s.astype(np.int64) + t.astype(np.int64)
    y = xi @ w.astype(np.int64)
    if bias is not None:
        y = y + bias.astype(np.int64)
    return np.maximum(y, 0) if act == 1 else y


def abs_terms(x, s, t, w, bias):
    """sum_c |x'_c w_cj| + |bias_j| in float64"""
    xp = x.astype(np.float64) if s is None else x.astype(np.float64) * s.astype(np.float64) + t.astype(np.float64)
    return np.abs(xp) @ np.abs(w.astype(np.float64)) + (0.0 if bias is None else np.abs(bias.astype(np.float64)))


def preact(x, s, t, w, bias):
    xp = x.astype(np.float64) if s is None else x.astype(np.float64) * s.astype(np.float64) + t.astype(np.float64)
    return xp @ w.astype(np.float64) + (0.0 if bias is None else bias.astype(np.float64))


def f64(x, s, t, w, bias, act):
    """float64 result on the stored fp32 operands"""
    v = preact(x, s, t, w, bias)
    return np.maximum(v, 0.0) if act == 1 else 1.0 / (1.0 + np.exp(-v)) if act == 2 else v


def sigmoid_bound(v):
    """error of 1 / (1 + __expf(-v)) at the fp32 pre-activation: the SE gate's figure of tests/sweeps_ref.py (se_ref: d_g)"""
    return (np.abs(v) + 8.0) * EPS32


def bound(x, s, t, w, bias, act):
    Cin = x.shape[1]
    b = (Cin + 3) * EPS32 * abs_terms(x, s, t, w, bias)
    if s is not None:
        xd = x.astype(np.float64)
        b = b + 2 * EPS32 * ((np.abs(xd * s.astype(np.float64)) + np.abs(t.astype(np.float64))) @ np.abs(w.astype(np.float64)))
    if act == 2:
        b = b / 4 + sigmoid_bound(preact(x, s, t, w, bias))
    return b
