"""Scalar reference of sdk_resample_s16 (csrc/resample.hip) in Python integers, and the fixtures its CPU and GPU tests share.

The documented formula (include/sdk_hip.h, oracle/resample.py), evaluated one output at a time with arbitrary-precision ints and no numpy
arithmetic - numpy only hands over the values (`.tolist()`):

    mono[i] = floor((sum_c x[i][c] + C // 2) / C)             samples outside [0, n_in) are zero
    acc[n]  = sum_k taps[(n M) mod L][k] * mono[floor(n M / L) + k - K/2 + 1]
    y[n]    = clamp((acc[n] + 2^29) >> 30, -32768, 32767)

oracle/resample.py is a vectorised int64 restatement of the same formula; tests/test_resample_ref_cpu.py ties the two together, and the GPU
tests compare every output with the oracle and a sampled set (`sample_indices`) with this file.

The fixtures are plain functions of seeds, so the CPU file can assert on the reference alone what each GPU test relies on (that a saturation
input really leaves the s16 range on both sides, and so on).
"""
from __future__ import annotations

from operator import mul

import numpy as np

PER_WG = 2048          # outputs per workgroup (RS_PER_WG of csrc/resample.hip): 2046..2050 and 4094..4098 straddle its edges
LDS_LIMIT = 65536      # an operand is staged in LDS when it fits in this many bytes

# (L, M, K), rate_in (None: synthetic taps straight to the C ABI; else designed for rate_in -> 16000 Hz), taps in LDS, window in LDS
CASES = [
    ((1, 1, 2), None, True, True),             # smallest
    ((2, 3, 8192), None, True, True),          # table at its limit: 65536 B exactly
    ((4100, 3, 4), None, False, True),         # table just over: 65600 B
    ((1, 16, 14), None, True, True),           # window at its limit: 65536 B exactly
    ((1, 16, 16), None, True, False),          # window just over: 65540 B
    ((1, 17, 2), None, True, False),           # K = 2 on the global window
    ((4097, 70000, 4), None, False, False),    # both global
    ((8, 125, 500), 250000, True, True),       # largest LDS image (16000 + 64972 B): needs the opt-in above 64 KiB
    ((20, 441, 706), 352800, True, False),     # real rate on <true, false>
    ((80, 1323, 530), 264600, False, False),   # real rate on <false, false>
    ((1, 24, 768), 384000, True, False),       # real rate on <true, false>
]
SYNTHETIC = [c[0] for c in CASES if c[1] is None]
DESIGNED = [(c[0], c[1]) for c in CASES if c[1] is not None]
# forced saturation: one designed or synthetic table on each of the four paths, and the two synthetic tables at the window limit.
# (K = 2 with L = 1 is one random phase whose sum of |h| need not exceed 2^30; K = 8192 saturates by ~4000x and costs seconds.)
SATURATION = [(8, 125, 500), (4100, 3, 4), (20, 441, 706), (80, 1323, 530), (4097, 70000, 4), (1, 16, 14), (1, 16, 16)]
CHANNELS = (1, 2, 3, 5, 7, 64)
ROUNDING_TABLES = {"half": [[1 << 29, 0]], "neg_half": [[-(1 << 29), 0]], "sum": [[1 << 30, 1 << 30]]}


def case_id(shape) -> str:
    return "L%d_M%d_K%d" % tuple(shape)


def plan_bits(L: int, M: int, K: int) -> int:
    """What sdk_resample_plan must return, from the rule as the header states it: bit 0 taps in LDS, bit 1 window in LDS."""
    tab = 4 * L * K
    win = ((2047 * M // L + K + 2) * 2 + 3) & ~3
    return (1 if tab <= LDS_LIMIT else 0) | (2 if win <= LDS_LIMIT else 0)


# ------------------------------------------------------------------------------------------------ the scalar reference
def downmix(x) -> list:
    """x int16 [n] or [n, C] -> list of n Python ints: floor((sum_c x + C // 2) / C)."""
    x = np.asarray(x)
    if x.ndim == 1:
        return [int(v) for v in x.tolist()]
    C = x.shape[1]
    return [(sum(row) + C // 2) // C for row in x.tolist()]          # Python's // on ints is floor division


def accumulate_at(x, taps, L: int, M: int, idx) -> list:
    """The exact accumulators acc[n], n in idx, as Python ints."""
    mono = downmix(x)
    n_in = len(mono)
    h = np.asarray(taps).tolist()
    K = len(h[0])
    out = []
    for n in idx:
        n = int(n)
        i0, ph = divmod(n * M, L)
        ib = i0 - (K // 2 - 1)                                       # input sample under tap 0
        k0, k1 = max(0, -ib), min(K, n_in - ib)                      # taps that fall inside the signal; the rest meet zeros
        out.append(sum(map(mul, h[ph][k0:k1], mono[ib + k0:ib + k1])) if k0 < k1 else 0)
    return out


def round_shift(acc: int) -> int:
    """Round half up: (acc + 2^29) >> 30 on an arbitrary-precision int (>> floors, as an arithmetic shift does)."""
    return (acc + (1 << 29)) >> 30


def resample_raw_at(x, taps, L: int, M: int, idx) -> list:
    """The rounded values BEFORE the s16 clamp: a test shows with them that a clamp took place."""
    return [round_shift(a) for a in accumulate_at(x, taps, L, M, idx)]


def resample_at(x, taps, L: int, M: int, idx) -> list:
    """y[n], n in idx, as Python ints in the s16 range."""
    return [max(-32768, min(32767, v)) for v in resample_raw_at(x, taps, L, M, idx)]


def out_len(n_in: int, L: int, M: int) -> int:
    return -(-n_in * L // M)


# ------------------------------------------------------------------------------------------------ fixtures
def synthetic_taps(L: int, M: int, K: int) -> np.ndarray:
    """Seeded int32 in [-2^30, 2^30], no unit-gain normalisation (the kernel does not depend on it); |acc| <= K * 2^45 < 2^58 at K <= 8192."""
    rng = np.random.default_rng([L, M, K])
    return rng.integers(-(1 << 30), (1 << 30) + 1, (L, K)).astype(np.int32)


def noise(n: int, ch: int, seed) -> np.ndarray:
    """Full-scale seeded noise [n] (ch = 0) or [n, ch]; the first and the last sample are the two extremes, so a tap that wrongly skips or
    wrongly reads either end changes a result."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, (n, max(ch, 1))).astype(np.int16)
    x[0] = -32768
    x[-1] = 32767
    return x[:, 0].copy() if ch == 0 else x


def n_in_for(n_out: int, L: int, M: int) -> int:
    """The smallest n_in whose output has at least n_out samples: exactly n_out whenever L <= M (every length is reachable when decimating)."""
    return (n_out - 1) * M // L + 1


def lengths(L: int, M: int, K: int):
    """-> (n_in at the workgroup edges, n_in at the windows that hang over both ends at once), each sorted and without repeats."""
    edges = sorted({n_in_for(n, L, M) for n in (1, PER_WG - 1, PER_WG, PER_WG + 1, 2 * PER_WG + 1)})
    short = sorted({n for n in (1, 2, K // 2 - 1, K // 2, K, K + 1) if n >= 1})
    return edges, short


def sample_indices(n_out: int, K: int, seed=0) -> list:
    """The outputs compared with the scalar reference: the first and last K, those around the first two workgroup edges, 200 seeded ones."""
    rng = np.random.default_rng([n_out, K, seed])
    idx = set(range(min(K, n_out))) | set(range(max(0, n_out - K), n_out))
    idx |= {n for n in list(range(2046, 2051)) + list(range(4094, 4099)) if n < n_out}
    idx |= set(rng.integers(0, n_out, 200).tolist())
    return sorted(idx)


def saturation_input(taps, L: int, M: int, targets: int = 16):
    """-> (x int16 [n_in], target output indices).  Target j is the output j * step, step chosen so that the targets' input windows are
    disjoint; under target j's window x = s_j * 32767 * sign(h), s_j = +1, -1, +1, ..: its accumulator is s_j * 32767 * sum|h|, the largest
    sum of that sign its phase can reach.  Everything else is full-scale noise."""
    h = np.asarray(taps).astype(np.int64)
    K = h.shape[1]
    step = -(-(K + 1) * L // M) + 1                                  # step * M / L - 1 >= K: windows of neighbouring targets do not meet
    tg = [j * step for j in range(targets)]
    n_in = n_in_for(tg[-1] + step, L, M)
    x = noise(n_in, 0, [L, M, K, 77]).astype(np.int64)
    for j, n in enumerate(tg):
        i0, ph = divmod(n * M, L)
        ib = i0 - (K // 2 - 1)
        k = np.arange(max(0, -ib), min(K, n_in - ib))
        x[ib + k] = (1 if j % 2 == 0 else -1) * 32767 * np.sign(h[ph, k])
    return x.astype(np.int16), tg


def all_s16_values() -> np.ndarray:
    """Every s16 value in order, then every value again in a seeded order (neighbouring sums then vary), then six samples whose
    neighbouring sums are 32768, 32767, -32768 and -32769, the four values next to the clamps: 131078 samples."""
    v = np.arange(-32768, 32768, dtype=np.int16)
    return np.concatenate([v, np.random.default_rng(5).permutation(v), np.array([1, 32767, 0, -32768, -1, 0], dtype=np.int16)])


def downmix_input(C: int, blocks: int = 24, stride: int = 17) -> np.ndarray:
    """[blocks * stride, C] of full-scale noise with the rounding rows at the frames 0, stride, 2 stride, ..: the run that keeps every
    17th down-mixed sample (L, M, K = 1, 17, 2) sees them all.  Rows: all -32768, all 32767, alternating extremes, and sums of
    -1, -(C // 2), -(C // 2) - 1 and C // 2 made of one balancing sample and small random ones."""
    rng = np.random.default_rng([C, 31])
    x = noise(blocks * stride, C, [C, 32])
    rows = [np.full(C, -32768), np.full(C, 32767), np.where(np.arange(C) % 2 == 0, -32768, 32767)]
    for s in (-1, -(C // 2), -(C // 2) - 1, C // 2):
        r = rng.integers(-300, 301, C)                               # 63 * 300 < 32768: the balancing sample stays in range
        r[0] = s - r[1:].sum()
        rows.append(r)
    for j, r in enumerate(rows):
        x[j * stride] = r
    x[-1] = 32767                                                    # the last frame keeps its extreme
    return x
