"""The embedding widths at which the second column of a thread is live for a part of the workgroup only, and the condition that makes a
test at such a width worth its time.

A 256-thread workgroup that gives thread tid the columns tid and tid + 256 (or a lane the columns lane + 64 q) has, at 256 < d < 512, waves
whose guard `tid + 256 < d` holds and waves whose guard fails: at d = 320 = 256 + one wave only wave 0 has a second column, at
d = 448 = 512 - one wave every wave but the last.  The shipped widths (192, 256, 512) never reach that state.

A case at such a width says something only if the columns FIRST.. carry weight in what is compared.  `weight` states that on the reference
alone: the reference is evaluated a second time on the input with the columns FIRST.. set to zero - what a kernel that lost its second column
would have read - and must then give other integers, or floats further away than FAR times the case's bound."""
from __future__ import annotations

import numpy as np

FIRST = 256                       # columns below it belong to a thread's first column
WIDTHS = (320, 448)               # 256 + one wave, 512 - one wave
FAR = 100.0


def first_columns(x) -> np.ndarray:
    """A copy of x [.., d] with the columns FIRST.. set to zero."""
    out = np.array(x, copy=True)
    out[..., FIRST:] = 0
    return out


def weight(name: str, ints=(), floats=(), bound: float = 0.0) -> float:
    """ints, floats: pairs (of the full input, of its first columns alone) of the reference's integer and float outputs.  Prints and returns
    the largest float distance over the bound (inf when an integer output differs) and asserts the condition above."""
    differ = any(not np.array_equal(a, b) for a, b in ints) or any(np.shape(a) != np.shape(b) for a, b in floats)       # another shape: another count
    far = max((float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) for a, b in floats if np.size(a) and np.shape(a) == np.shape(b)),
              default=0.0)
    ratio = far / bound if bound > 0 else (np.inf if far > 0 else 0.0)
    print(f"{name}: without the columns {FIRST}.. the reference's integers {'differ' if differ else 'are the same'}; its floats move by {far:.3e}, "
          f"{ratio:.3e} x the bound {bound:.3e} (must exceed {FAR:g} x unless the integers differ)")
    assert differ or ratio > FAR, f"{name}: the columns {FIRST}.. carry no weight in this case: choose another seed"
    return np.inf if differ else ratio
