"""float64 model of the precise mode's fp16 hi + lo plane pair (csrc/hp.hpp) and restatements of its four sweeps (csrc/hp.hip:
seg_mean_hp, se_apply_hp, asp_stats_hp, asp_pool_hp) for tests/test_hp_sweeps_gpu.py.  Every restatement takes the DECODED planes
(float64) and returns the exact value next to a bound on the kernel's fp32 error, n 2^-24 sum|terms| with n read off the kernel's own
summation order (stated at each function).  tests/test_hp_ref_cpu.py checks the pair model against Engine.to_planes and the
restatements against oracle/ecapa.py."""
import torch

import sweeps_ref as R

EPS32 = R.EPS32
LOSCALE = 2048.0
HP_MAX = 65504.0
SENT = -7.75            # sentinel around every operand and output: exact in both planes (hi = -7.75, a lo of -7.75 decodes exactly too)


# ---------------------------------------------------------------------------------------------------- the pair
def split(v):
    """split1 of csrc/hp.hpp in fp32: saturate at +-65504, hi = fp16(v), lo = fp16((v - hi) * 2^11) -> (hi, lo) fp16 tensors"""
    v = torch.as_tensor(v).float().clamp(-HP_MAX, HP_MAX)
    hi = v.to(torch.float16)
    lo = ((v - hi.float()) * LOSCALE).to(torch.float16)
    return hi, lo


def join(hi, lo):
    """the value a pair holds, exactly: hi + lo / 2^11 in float64 (11 + 11 bits, 11 binary places apart: no rounding)"""
    return hi.double() + lo.double() / LOSCALE


def decode(v):
    """what the planes hold of an fp32 tensor: join(split(v))"""
    return join(*split(v))


def storage_bound(v):
    """|join(split(v)) - v| <= 2^-22 |v| + 2^-36 for a stored fp32 v, |v| <= 65504.  |v - hi| <= 2^-11 |v| (fp16's 11 bits; below 2^-14,
    where hi is subnormal, <= 2^-25), the residual and its scaling by 2^11 are exact in fp32, and the scaled lo rounds with relative
    error 2^-11 in fp16's normal range (2^-11 2^-11 |v|) or with absolute error 2^-25 in the subnormal range (2^-36 unscaled)."""
    return 2.0 ** -22 * torch.as_tensor(v, dtype=torch.float64).abs() + 2.0 ** -36


def planes(v, ld, lo, rows_extra=0):
    """fp32 [rows, C] -> fp16 buffer [rows + rows_extra, ld] filled with SENT, hi plane in columns [0, C), lo plane in [lo, lo + C).
    The operand is buf[:rows] with lo offset `lo`; the sentinel columns to the right of each plane are there to be read by a kernel
    that runs past C."""
    rows, C = v.shape
    assert lo >= C and ld >= lo + C
    buf = torch.full((rows + rows_extra, ld), SENT, dtype=torch.float16)
    hi, l = split(v)
    buf[:rows, :C] = hi
    buf[:rows, lo:lo + C] = l
    return buf


# ---------------------------------------------------------------------------------------------------- the sweeps
def seg_mean_ref(z, B, T):
    """[B, C] mean over frames.  seg_mean_hp_kernel: join is exact in fp32 for a pair that split made; four frame groups sum their
    ceil(T / 4) strided frames in sequence (ceil(T / 4) - 1 rounded adds), three adds merge them, then * (1 / T) with 1 / T itself
    rounded: ceil(T / 4) + 4 roundings on a term's path, n = ceil(T / 4) + 5 (one for the second order)."""
    zb = z.double().reshape(B, T, -1)
    n = -(-T // 4) + 5
    return zb.mean(1), n * EPS32 * zb.abs().mean(1)


def se_apply_ref(z, x, gate, B, T):
    """g * z + x on GIVEN fp32 gates [B, C], then the pair store.  Returns (target, bound, value before saturation, arithmetic
    bound) [B*T, C]: se_apply_hp_kernel rounds the product and the sum (or one fused multiply-add): 2 2^-24 (|g z| + |x|); split1
    then saturates at +-65504 and stores within storage_bound of the kernel's own fp32 value, which is within the arithmetic bound
    of the exact one."""
    C = z.shape[1]
    zb, xb = z.double().reshape(B, T, C), x.double().reshape(B, T, C)
    gz = gate.double()[:, None, :] * zb
    want = (gz + xb).reshape(B * T, C)
    acc = (2 * EPS32 * (gz.abs() + xb.abs())).reshape(B * T, C)
    tgt = want.clamp(-HP_MAX, HP_MAX)
    return tgt, acc + storage_bound(tgt.abs() + acc), want, acc


def asp_stats_ref(h, B, T):
    """[B, 2C] mean | sqrt(max(var, 1e-12)): the value of sweeps_ref.asp_stats_ref, the bound in its form with the sums of
    asp_stats_hp_kernel.  d = h - K, K = frame 0, is rounded once; two frame groups sum their ceil(T / 2) strided d in sequence,
    one add merges them, * (1 / T) with 1 / T rounded: ceil(T / 2) + 3 roundings on a term of the mean, n = ceil(T / 2) + 4; the mean
    is K + a: one more rounding of |mu| (written 2, as sweeps_ref does).  Second moment q: d^2 carries d's rounding twice, the
    multiply-add rounds once more: (n + 2) 2^-24 m2, m2 = mean d^2; a^2: 2 |a| e_a + 2^-24 a^2 <= (2 n + 1) 2^-24 m2 (|a| mean|d| <=
    m2); the subtraction q - a^2 rounds var <= m2 once: e_var = (3 n + 4) 2^-24 m2."""
    C = h.shape[1]
    want, _ = R.asp_stats_ref(h, B, T)
    hb = h.double().reshape(B, T, C)
    mu = want[:, :C]
    var = ((hb - mu[:, None]) ** 2).mean(1)
    d = hb - hb[:, :1]
    n = -(-T // 2) + 4
    e_mu = n * EPS32 * d.abs().mean(1) + 2 * EPS32 * mu.abs()
    e_var = (3 * n + 4) * EPS32 * (d ** 2).mean(1)
    return want, torch.cat([e_mu, R.sqrt_bound(var, e_var)], 1)


def rescales_after(lg):
    """[B, T, C] the number of frames j > t at which asp_pool_hp_kernel's running maximum grows (l_j > max_{i < j} l_i, compared in
    fp32 as the kernel does): how many times frame t's contribution is rescaled"""
    run = torch.cummax(lg, 1).values
    grows = torch.zeros_like(lg)
    grows[:, 1:] = (lg[:, 1:] > run[:, :-1]).to(lg.dtype)
    total = grows.sum(1, keepdim=True)
    return total - torch.cumsum(grows, 1)


def asp_pool_ref(logits, h, B, T):
    """softmax over frames of the fp32 logits [B*T, C] -> weighted mean | std of h [B, 2C]: the value of sweeps_ref.asp_pool_ref,
    the bound in its form with the sums of asp_pool_hp_kernel - ONE chain over the T frames per channel: d = h - K (K = frame 0,
    rounded once), w = expf(l - mx), three fused multiply-adds, and where the running maximum grows the three running sums times
    expf(mx_old - mx_new).
    A weight's relative error dw: every exp argument is a difference of two fp32 values rounded once, and the arguments on frame t's
    way to the final maximum add up to mx - l_t (the maximum only grows): 2^-24 (mx - l_t); each expf is good to 1 ulp = 2 2^-24, one
    for the weight and one per rescale after t (R_t, counted from the logits).  It moves the mean by sum w dw |h - mu| and the
    variance by sum w dw |(h - mu)^2 - var|.
    Sums: a term of s1 meets T accumulations and R rescale multiplies (R = all rescales of the column), d's rounding and the
    division: n = T + R + 2, on the terms w |d| about K; the denominator carries the same n relatively: e_mu = 2 n 2^-24 sum w |d|
    + 2 2^-24 |mu| (K + a, written 2 as above).  Variance q - a^2 with m2 = sum w d^2: s2 (w d rounded, d^2 twice d's rounding) and
    its denominator (2 n + 2), a^2: 2 |a| e_a + 2^-24 a^2 <= (4 n + 1) m2, the division and the subtraction 2 more:
    e_var = (6 n + 5) 2^-24 m2, plus the mean's error squared."""
    C = h.shape[1]
    want, _ = R.asp_pool_ref(logits, h, B, T)
    lg = logits.double().reshape(B, T, C)
    hb = h.double().reshape(B, T, C)
    w = torch.softmax(lg, 1)
    mu = want[:, :C]
    dev = hb - mu[:, None]
    var = (w * dev ** 2).sum(1)
    d = hb - hb[:, :1]
    mx = lg.max(1, keepdim=True).values
    r_after = rescales_after(lg)
    dw = EPS32 * (mx - lg) + 2 * EPS32 * (1 + r_after)
    n = T + r_after[:, 0] + 2
    e_w = (w * dw * dev.abs()).sum(1)
    e_mu = e_w + 2 * n * EPS32 * (w * d.abs()).sum(1) + 2 * EPS32 * mu.abs()
    e_var = (w * dw * (dev ** 2 - var[:, None]).abs()).sum(1) + (6 * n + 5) * EPS32 * (w * d ** 2).sum(1) + e_mu ** 2
    return want, torch.cat([e_mu, R.sqrt_bound(var, e_var)], 1)
