"""References for csrc/fbank.hip that need neither a GPU nor torch (numpy and oracle/fbank.py only).

Used by tests/test_fbank_cpu.py (which checks, without a device, the conditions the GPU file relies on) and by
tests/test_fbank_gpu.py.  Three things live here:

  inputs(S)            the int16 rows (a)..(g) at one of the lengths in SHAPES, seeded: both files see the same bytes
  raw_interval(pcm)    per element an interval that the kernel's fp32 log-mel (before floor and mean) must lie in, derived
                       below from the kernel's arithmetic and evaluated from the float64 oracle alone
  norm_fp32(L, ...)    the two normaliser kernels restated operation by operation in IEEE fp32: equal to the device bit for bit

Nothing in this file was fitted to a device result.

Derivation of raw_interval
--------------------------
Notation: u = 2^-24 (unit roundoff of fp32, round to nearest).  Frame t of a row holds x[0..399] (zero padded), w is the Hamming
window, A_t = sum_n w[n] |x[n]| and U_t = sum_n |x[n]|.  The kernel folds K: e[n] = x[n] +- x[400-n], n = 0..200, against the table
c[n] = h_n w[n] cos / -w[n] sin (h_0 = h_200 = 1/2); since w[n] = w[400-n], sum_n |e[n]| |c[n]| <= A_t for the cos and the sin sum alike.

1. Samples.  e[n] is an integer of at most 17 bits times 2^-15 and exact in fp32.  A format of p significand bits rounds with a
   relative error of at most 2^-p (half an ulp).  bf16 (p = 8): hi = RNE(e) leaves an integer residual of at most 2^7 in the same
   unit, which has 8 bits: e = hi + lo EXACTLY, with |lo| <= 2^-8 |e|.  fp16 (p = 11): |e| <= 2, so the residual is a multiple of
   2^-15 of at most 2^-11, i.e. at most 5 bits (subnormal below 2^-14, representable): exact again, |lo| <= 2^-11 |e|.  No term.
   (If a split were not exact on the device, rows (d) and (f) would leave the interval.)
2. Table residual.  chi = RNE_p(c), clo = RNE_p(c - chi), each taken through one extra rounding to fp32 or from float64:
   |c - chi| <= 2^-p |c| (1 + 2^-14), and the same again for clo against the residual, so |c - chi - clo| <= 1.001 * 2^-2p |c|.
   bf16 has fp32's exponent range; fp16 is subnormal below 2^-14, where clo is only good to half the subnormal quantum, 2^-25
   ABSOLUTE - that term multiplies U_t instead of A_t.
       d_table <= 1.001 * 2^-2p A_t  (+ 2^-25 U_t for fp16)
3. The dropped product lo.lo:  |e_lo| |c_lo| <= 2^-p |e| * 2^-p |c| * 1.001:
       d_lolo  <= 1.001 * 2^-2p A_t
4. fp32 accumulation.  The products of two p-bit numbers are exact in fp32 (2p <= 22 bits).  One accumulator takes 13 k-steps x 3
   matrix instructions x 16 products = 624 additions.  How the matrix unit orders the 16 additions of one instruction is not
   documented, so the bound used is the one that holds for EVERY order: (number of additions) * u * (sum of the absolute terms),
   the absolute terms being sum |e_hi c_hi| + |e_hi c_lo| + |e_lo c_hi| <= ((1 + 2^-p)^2 + 2 * 2^-p (1 + 2^-p)) A_t <= 1.02 A_t:
       d_acc   <= 624 * 1.02 * u * A_t
   This worst case is the largest item of the budget (636.5 u = 2^-14.7 against 2^-15 for items 2 + 3 with bf16).  It is kept
   although a random-walk estimate would be some 20 times smaller, because tests/test_fbank_cpu.py shows that even so a table
   without its lo plane leaves the interval: the bound has teeth as it stands and carries no confidence factor.
   Together:  |dRe|, |dIm| <= d_t = EPS[p] A_t + EPS_ABS[p] U_t,  EPS[bf16] = 2 * 1.001 * 2^-16 + 636.5 u = 2^-13.8,
   EPS[fp16] = 2 * 1.001 * 2^-22 + 636.5 u = 2^-14.7, EPS_ABS[fp16] = 2^-25.
5. Power.  P = fl(Re^2 + Im^2): two or three roundings of non-negative terms (with or without a fused multiply-add), so
   P in [ (max(|Re|-d,0)^2 + max(|Im|-d,0)^2)(1-3u), ((|Re|+d)^2 + (|Im|+d)^2)(1+3u) ].
6. Mel.  acc += P[f] * melw[f] over the n_m bins of filter m in fp32: melw is the float64 weight rounded once (u), each product
   rounds once (u), the chain adds n_m times; all terms are non-negative, so the relative error is at most (n_m + 2) u, plus
   the 3u of item 5: M in [M(P_lo) (1 - (n_m+5)u), M(P_hi) (1 + (n_m+5)u)].  The device builds its filter corners as
   lo + (hi - lo) i / 81 where the oracle uses linspace: weights differ by ~1e-15 absolute, and a bin that sits exactly on a corner
   may carry such a weight on one side only.  Covered by +-2^-40 * (sum of the frame's P_hi) on M, absolutely.
7. Guard and log.  fmaxf(acc, 1e-10f): the fp32 constant is within u of 1e-10, i.e. 4.35 u dB, added to the log term.
   Default / precision 2: 3.0102999566f * v_log_f32(x).  The instruction is specified to 1 ulp; its ulp is taken at a magnitude of at
   least 1 (2^-23 absolute) so that nothing is claimed about relative accuracy next to log2(1) = 0.  The constant is within u of
   10 log10(2) and the product rounds once:  dL <= 3.0103 * 2^-23 max(|log2 x|, 1) + 2 u |L|  (at most 1.3e-5 + 1.2e-5 dB).
   Precision 1: 10.0f * log10f(x), the device library's log10f at its documented 2 ulp (ulp taken at a magnitude of at least 2^-3),
   one rounding for the product:  dL <= 10 * 2 * 2^-23 max(|log10 x|, 2^-3) + u |L| = 2 * 2^-23 max(|L|, 1.25) + u |L|.
   The log terms are added in dB on both ends AFTER the guard, so the guard is kept on both ends as the kernel applies it.
"""
from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import fbank as ofbank  # noqa: E402

U32 = 2.0 ** -24
FT = 32                     # frames per tile of fbank_tile_kernel
NORM_LDS_MAX_T = 480        # last T on fbank_norm_lds_kernel
N_MELS = ofbank.N_MELS
HOP = ofbank.HOP

# S -> T = 1 + S // 160: one frame, two frames, the tile edge (32 | 33), the switch between the two normalisers (480 | 481)
SHAPES = (1, 159, 160, 4960, 5119, 5120, 76640, 76800)
ROWS = "abcdefg"
FLOOR_ROWS = (0, 1, 4)      # (a), (b), (e): the rows whose floor engages

N_ADDS = 13 * 3 * 16
EPS = {0: 2 * 1.001 * 2.0 ** -16 + N_ADDS * 1.02 * U32, 1: 2 * 1.001 * 2.0 ** -22 + N_ADDS * 1.02 * U32}
EPS_ABS = {0: 0.0, 1: 2.0 ** -25}
EPS[2], EPS_ABS[2] = EPS[0], EPS_ABS[0]          # precision 2 runs the default tile kernel: only the storage format differs


def _q(x: np.ndarray) -> np.ndarray:
    return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)


def inputs(S: int, seed: int = 17) -> np.ndarray:
    """[7, S] int16, rows (a)..(g) in this order (ROWS):
    (a) 440 Hz at 0.5 over the first half, digital silence after;  (b) noise at 0.1 with ~2000 samples zeroed from an offset that is
    no multiple of the hop;  (c) all zeros;  (d) full-scale two-level noise, -32768 / 32767;  (e) DC at 0.25;  (f) 300 Hz at 0.5 over
    noise at 1e-4;  (g) the recipe of test_gpu_kernels._pcm (noise at 0.1 plus two tones), the control whose floor never engages."""
    t = np.arange(S) / 16000.0
    rng = [np.random.default_rng([seed, S, r]) for r in range(len(ROWS))]
    a = 0.5 * np.sin(2 * np.pi * 440.0 * t)
    a[S // 2:] = 0.0
    b = rng[1].normal(0, 0.1, S)
    z0 = (S // 3) | 1                                        # odd: never a multiple of 160
    b[z0:z0 + 2001] = 0.0
    c = np.zeros(S)
    d = np.where(rng[3].integers(0, 2, S) == 1, 32767.0, -32768.0) / 32768.0
    if S >= 2:
        d[0], d[-1] = -1.0, 32767.0 / 32768.0                # both levels present at every length
    e = np.full(S, 0.25)
    f = 0.5 * np.sin(2 * np.pi * 300.0 * t) + rng[5].normal(0, 1e-4, S)
    g = rng[6].normal(0, 0.1, S) + 0.2 * np.sin(2 * np.pi * (200 + 37 * 6) * t) + 0.1 * np.sin(2 * np.pi * (1800 + 91 * 6) * t)
    return np.stack([_q(r) for r in (a, b, c, d, e, f, g)])


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def case(S: int):
    """(pcm, raw_logmel64(pcm)) of a length in SHAPES, computed once per process and read-only."""
    pcm = inputs(S)
    return _frozen(pcm, raw_logmel64(pcm))


@functools.lru_cache(maxsize=None)
def case_interval(S: int, precision: int):
    """raw_interval of case(S), once per process; precision 2 runs the default tile kernel and shares precision 0's interval."""
    if precision == 2:
        return case_interval(S, 0)
    return _frozen(*raw_interval(case(S)[0], precision))


@functools.lru_cache(maxsize=None)
def case_features(S: int):
    """oracle.fbank of case(S) as float64, once per process."""
    return _frozen(ofbank.fbank(case(S)[0]).astype(np.float64))


def mel_power64(pcm: np.ndarray, dft_bits=None) -> np.ndarray:
    return ofbank.power_spectrum(pcm, dft_bits) @ ofbank.mel_matrix()


def raw_logmel64(pcm: np.ndarray, dft_bits=None) -> np.ndarray:
    """The oracle's 10 log10(max(M, 1e-10)) before floor and mean: [B, T, 80] float64."""
    return 10.0 * np.log10(np.maximum(mel_power64(pcm, dft_bits), ofbank.AMIN))


def raw_interval(pcm: np.ndarray, precision: int = 0):
    """(L_lo, L_hi), [B, T, 80] float64 each: see the module docstring.  precision 0 / 2: bf16 table and the hardware log2;
    1: fp16 table and the library log10f."""
    C, Sn = ofbank.dft_matrices()
    fr = ofbank.frames_of(pcm)
    w = ofbank.hamming_window()
    re, im = np.abs(fr @ C), np.abs(fr @ Sn)
    afr = np.abs(fr)
    d = (EPS[precision] * (afr @ w) + EPS_ABS[precision] * afr.sum(axis=-1))[..., None]
    p_lo = (np.maximum(re - d, 0.0) ** 2 + np.maximum(im - d, 0.0) ** 2)
    p_hi = ((re + d) ** 2 + (im + d) ** 2)
    W = ofbank.mel_matrix()
    n_m = (W > 0).sum(axis=0).astype(np.float64)
    corner = 2.0 ** -40 * p_hi.sum(axis=-1, keepdims=True)
    m_lo = np.maximum((p_lo @ W) * (1.0 - (n_m + 5) * U32) - corner, 0.0)
    m_hi = (p_hi @ W) * (1.0 + (n_m + 5) * U32) + corner
    l_lo = 10.0 * np.log10(np.maximum(m_lo, ofbank.AMIN))
    l_hi = 10.0 * np.log10(np.maximum(m_hi, ofbank.AMIN))

    def dlog(L):
        if precision == 1:
            return 2 * 2.0 ** -23 * np.maximum(np.abs(L), 1.25) + U32 * np.abs(L) + 4.35 * U32
        log2x = np.abs(L) / (10.0 * np.log10(2.0))
        return 10.0 * np.log10(2.0) * 2.0 ** -23 * np.maximum(log2x, 1.0) + 2 * U32 * np.abs(L) + 4.35 * U32
    return l_lo - dlog(l_lo), l_hi + dlog(l_hi)


# ------------------------------------------------------------------------------------------------ storage formats
def bf16_bits(x32: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 bit patterns, round to nearest even (finite inputs)."""
    b = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32)
    return ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_value(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


def fp16_bits(x32: np.ndarray) -> np.ndarray:
    """fp32 -> fp16 bit patterns, saturated to +-65504 first as pack2t<true> does, round to nearest even."""
    return np.clip(np.asarray(x32, dtype=np.float32), np.float32(-65504.0), np.float32(65504.0)).astype(np.float16).view(np.uint16)


def planes_bits(x32: np.ndarray):
    """Engine.to_planes / sdk_hp::split1 in fp32: hi = fp16(sat(x)), lo = fp16((x - float(hi)) * 2^11)."""
    x = np.clip(np.asarray(x32, dtype=np.float32), np.float32(-65504.0), np.float32(65504.0))
    hi = x.astype(np.float16)
    lo = ((x - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def decode(bits: np.ndarray, fmt: str) -> np.ndarray:
    """Stored bit patterns [..., ldf] -> the float64 values of the 80 mel channels."""
    if fmt == "bf16":
        return bf16_value(bits[..., :N_MELS]).astype(np.float64)
    if fmt == "fp16":
        return bits[..., :N_MELS].view(np.float16).astype(np.float64)
    h = bits.shape[-1] // 2
    return bits[..., :N_MELS].view(np.float16).astype(np.float64) + bits[..., h:h + N_MELS].view(np.float16).astype(np.float64) / 2048.0


FMT = {0: "bf16", 1: "planes", 2: "fp16"}


# ------------------------------------------------------------------------------------------------ the normaliser in fp32
def norm_values_fp32(L32: np.ndarray, peak_of=None, clamp_in_mean: bool = True) -> np.ndarray:
    """fbank_norm_kernel / fbank_norm_lds_kernel up to the store, every operation in IEEE fp32 and in the kernels' order:
         flo   = max over the segment - 80.0f
         pv    = fmaxf(L[0, m], flo)                                                                (the bin's first frame)
         r_g   = sum of (fmaxf(L[t, m], flo) - pv) over t = g, g + 3, ... in this order, from 0.0f    (g = 0, 1, 2)
         mean  = pv + ((r_0 + r_1) + r_2) / (float)T
         value = fmaxf(L[t, m], flo) - mean
    The sums run over differences from the first frame so that a bin that is constant over the segment (digital silence) gets features
    of exactly 0: the plain sum of T equal values, divided by T, is one ulp off at some T.
    [B, T, 80] fp32 in and out.  The two keyword arguments exist for the wrong-order mutants of tests/test_fbank_cpu.py only:
    peak_of(L) -> [B, T, 1] replaces the segment's peak; clamp_in_mean = False takes the mean before the clamp."""
    L = np.asarray(L32, dtype=np.float32)
    assert L.dtype == np.float32 and L.ndim == 3 and L.shape[2] == N_MELS
    B, T, _ = L.shape
    peak = L.reshape(B, -1).max(axis=1)[:, None, None] if peak_of is None else peak_of(L)
    flo = (peak - np.float32(80.0)).astype(np.float32)
    clamped = np.maximum(L, flo)
    src = clamped if clamp_in_mean else L
    pv = src[:, 0, :]
    r = np.zeros((3, B, N_MELS), dtype=np.float32)
    for t in range(T):
        r[t % 3] = r[t % 3] + (src[:, t, :] - pv)
    mean = pv + ((r[0] + r[1]) + r[2]) / np.float32(T)
    out = clamped - mean[:, None, :]
    assert out.dtype == np.float32
    return out


def norm_fp32(L32: np.ndarray, fmt: str, ldf: int) -> np.ndarray:
    """The stored features as 16-bit patterns [B, T, ldf]: norm_values_fp32 in the given format ("bf16", "fp16", or "planes":
    hi in columns [0, ldf / 2), lo * 2^11 in [ldf / 2, ldf)); channels 80 and up of every plane are +0."""
    v = norm_values_fp32(L32)
    B, T, _ = v.shape
    out = np.zeros((B, T, ldf), dtype=np.uint16)
    if fmt == "bf16":
        out[..., :N_MELS] = bf16_bits(v)
    elif fmt == "fp16":
        out[..., :N_MELS] = fp16_bits(v)
    elif fmt == "planes":
        assert ldf % 16 == 0 and ldf // 2 >= N_MELS
        hi, lo = planes_bits(v)
        out[..., :N_MELS] = hi
        out[..., ldf // 2:ldf // 2 + N_MELS] = lo
    else:
        raise ValueError(fmt)
    return out


def peak_per_tile(L: np.ndarray) -> np.ndarray:
    """Mutant: the peak of each 32-frame tile instead of the segment's."""
    B, T, _ = L.shape
    pk = np.empty((B, T, 1), dtype=np.float32)
    for t0 in range(0, T, FT):
        pk[:, t0:t0 + FT, 0] = L[:, t0:t0 + FT, :].reshape(B, -1).max(axis=1)[:, None]
    return pk


def norm_bound(T: int, L: np.ndarray) -> float:
    """fp32 summation over T frames in three chains: (T / 3 + 3) 2^-24 max |L|."""
    return (T / 3.0 + 3.0) * U32 * float(np.abs(L).max())


# ------------------------------------------------------------------------------------------------ end to end
def feature_interval(l_lo: np.ndarray, l_hi: np.ndarray, fmt: str):
    """The raw interval carried through floor, mean and store: every step of the normaliser is monotone in each input, so interval
    arithmetic is exact for it.  peak in [max l_lo, max l_hi]; clamped c in [max(l_lo, flo_lo), max(l_hi, flo_hi)]; mean in
    [mean c_lo, mean c_hi]; value in [c_lo - mean_hi, c_hi - mean_lo].  Widened by the normaliser's own fp32 error - the chain bound
    of norm_bound plus one rounding each for flo and the final difference, (T / 3 + 5) u max(|L|, |flo|) - and by half an ulp of the
    storage format at the bound's magnitude (bf16 2^-8, fp16 2^-11 relative or the subnormal 2^-25, planes 2^-22 relative or 2^-36).
    Returns (lo, hi, sure): sure marks the elements that are clamped whatever the error (l_hi < flo_lo)."""
    B, T, _ = l_lo.shape
    flo_lo = l_lo.reshape(B, -1).max(axis=1)[:, None, None] - 80.0
    flo_hi = l_hi.reshape(B, -1).max(axis=1)[:, None, None] - 80.0
    c_lo, c_hi = np.maximum(l_lo, flo_lo), np.maximum(l_hi, flo_hi)
    lo = c_lo - c_hi.mean(axis=1, keepdims=True)
    hi = c_hi - c_lo.mean(axis=1, keepdims=True)
    mag = np.maximum(np.abs(l_lo).reshape(B, -1).max(axis=1)[:, None, None], np.abs(flo_lo))
    e = (T / 3.0 + 5.0) * U32 * mag
    a = np.maximum(np.abs(lo), np.abs(hi)) + e
    half = {"bf16": 2.0 ** -8 * a, "fp16": np.maximum(2.0 ** -11 * a, 2.0 ** -25), "planes": np.maximum(2.0 ** -22 * a, 2.0 ** -36)}[fmt]
    return lo - e - half, hi + e + half, l_hi < flo_lo
