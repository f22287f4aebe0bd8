"""The one argument checker of the host wrappers (ops.py, ops_*.py, diarize_ops.py, resnet.py, score.py): the kernels read their arguments
through bare pointers, so whatever a kernel cannot see - type, dtype, shape, strides, host or device memory - is refused here, before any
launch, with a ValueError of one form:

    <entry point>: <argument> must be a contiguous <dtype> device tensor [<shape>], got <what it got>

Refused in this order: not a tensor, dtype, rank or extent, strides, host memory - the device last (in rows and thin after their own rules
too), so that host tensors reach every other refusal.  A valid argument costs the comparisons only: the text is built when it is raised.

A leaf: it imports neither torch nor _lib with the module (diarize_ops.py imports it, and that imports without torch).
"""
from __future__ import annotations

import numbers
import sys

THIN_MAX = 32      # KV of csrc/spectral.hip: the widest [n, k] block (and the most centres) the thin helpers take
MAX_ROW_DIM = 512  # the widest row the row kernels (assignment, VBx, k-means, AS-norm, PLDA) serve: d = 64, 128, .. 512

_SHORT = {"float32": "fp32", "bfloat16": "bf16", "float16": "fp16"}


def _dtype_name(dtype) -> str:
    """'fp32', 'float64', 'int32', .. of a torch dtype or of its short name ('float32')."""
    name = str(dtype).rpartition(".")[2]
    return _SHORT.get(name, name)


def _is_dtype(t, dtype) -> bool:
    if isinstance(dtype, (tuple, list)):
        return any(_is_dtype(t, d) for d in dtype)
    return str(t.dtype) == "torch." + dtype if isinstance(dtype, str) else t.dtype == dtype


def _refuse(who: str, name: str, t, dtype, shape, contiguous: bool, strides: bool = False, tail: str = ""):
    names = [_dtype_name(d) for d in (dtype if isinstance(dtype, (tuple, list)) else (dtype,))]
    want = f"{who}: {name} must be a {'contiguous ' if contiguous else ''}{' or '.join(names)} device tensor"
    if shape is not None:
        want += " [" + ", ".join("*" if s is None else str(s) for s in shape) + "]"
    if not hasattr(t, "is_cuda"):
        raise ValueError(f"{want}, got {type(t).__name__}")
    got = f"got {list(t.shape)} {_dtype_name(t.dtype)}" + (f" with strides {list(t.stride())}" if strides else "") + ("" if t.is_cuda else f" on {t.device}")
    raise ValueError(f"{want}, {got}{tail}")


def _host_side(who: str, name: str, t, dtype, shape, contiguous: bool) -> None:
    """Every refusal but the device's."""
    torch = sys.modules.get("torch")                 # no torch in the process: no tensor either
    if torch is None or not isinstance(t, torch.Tensor) or not _is_dtype(t, dtype):
        _refuse(who, name, t, dtype, shape, contiguous)
    if shape is not None and (t.dim() != len(shape) or any(s is not None and s != m for s, m in zip(shape, t.shape))):
        _refuse(who, name, t, dtype, shape, contiguous)
    if contiguous and not t.is_contiguous():
        _refuse(who, name, t, dtype, shape, contiguous, strides=True, tail=f" (pass {name}.contiguous())")


def _on_device(who: str, name: str, t, dtype, shape, contiguous: bool) -> None:
    if not t.is_cuda:
        _refuse(who, name, t, dtype, shape, contiguous, tail=": there is no CPU path")


def tensor(who: str, name: str, t, dtype, shape=None, contiguous: bool = True):
    """`t`, argument `name` of entry point `who`, must be a tensor of `dtype` (a torch dtype, its short name such as "float32", or a tuple of
    either) and of `shape` (an int per extent, None for any extent; shape=None: any shape), contiguous (contiguous=False: the caller passes
    t.contiguous() on) and in device memory.  -> t"""
    _host_side(who, name, t, dtype, shape, contiguous)
    _on_device(who, name, t, dtype, shape, contiguous)
    return t


def row_width(who: str, d: int, limit: int = MAX_ROW_DIM) -> int:
    """The width of a row the row kernels serve: a multiple of 64, at most `limit`.  -> d"""
    if d < 64 or d % 64 or d > limit:
        raise ValueError(f"{who}: d={d} not supported (a multiple of 64, at most {limit})")
    return int(d)


def rows(who: str, name: str, t, n=None, d=None, limit: int = MAX_ROW_DIM):
    """A block of fp32 rows [n, d] (n, d None: any) of a served width -> (n, d)."""
    _host_side(who, name, t, "float32", (n, None), True)
    dd = row_width(who, int(t.shape[1]), limit)
    if d is not None and dd != d:
        raise ValueError(f"{who}: {name} has d={dd}, expected {d}")
    _on_device(who, name, t, "float32", (n, None), True)
    return int(t.shape[0]), dd


def thin(who: str, name: str, t):
    """The [n, k] row block of a thin helper (rows_gram .. kmeans_assign): fp32, contiguous, n >= 1, 1 <= k <= THIN_MAX -> (n, k)."""
    _host_side(who, name, t, "float32", (None, None), True)
    n, k = int(t.shape[0]), int(t.shape[1])
    if n < 1:
        raise ValueError(f"{who}: {name} must be [n, k] with n >= 1, got {list(t.shape)}")
    if not 1 <= k <= THIN_MAX:
        raise ValueError(f"{who}: k = {k} (the width of {name}) must be in 1..{THIN_MAX}")
    _on_device(who, name, t, "float32", (None, None), True)
    return n, k


KNN_P_MAX = 64     # KNN_P_MAX of csrc/nmesc.hip: the longest neighbour list, one lane per entry (cluster.NMESC_P_MAX)


def knn_shape(who: str, n: int) -> int:
    """The rows of a neighbour graph (knn_rows .. knn_matvec) -> P = min(KNN_P_MAX, n - 1)."""
    if n < 2 or n > 65536:
        raise ValueError(f"{who}: n={n} rows (2 .. 65536)")
    return min(KNN_P_MAX, n - 1)


def knn_lists(who: str, idx):
    """The neighbour lists idx int32 [n, P] with P = min(KNN_P_MAX, n - 1) -> (n, P)."""
    n, P = (int(v) for v in tensor(who, "idx", idx, "int32", (None, None)).shape)
    if knn_shape(who, n) != P:
        raise ValueError(f"{who}: idx must be [n, min({KNN_P_MAX}, n - 1)], got {list(idx.shape)}")
    return n, P


KNN_MAX_SCALES = 8     # KNN_MAX_SCALES of csrc/nmesc.hip: the scales of one fused affinity


def knn_maps(who: str, maps):
    """The maps of a fused affinity: int32 [S, n], 1 <= S <= KNN_MAX_SCALES, n a neighbour graph's rows -> (S, n, P)."""
    S, n = (int(v) for v in tensor(who, "maps", maps, "int32", (None, None)).shape)
    if not 1 <= S <= KNN_MAX_SCALES:
        raise ValueError(f"{who}: maps must be [S, n] with S in 1..{KNN_MAX_SCALES}, got {list(maps.shape)}")
    return S, n, knn_shape(who, n)


def knn_weights(who: str, weights, S: int):
    """The scale weights of a fused affinity: S host numbers, finite, >= 0, not all zero -> a list of S floats, as given (the caller
    normalises: cluster.nmesc_multiscale)."""
    try:
        w = [float(v) for v in weights]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: weights must be {S} host numbers, got {weights!r}") from None
    if len(w) != S or any(isinstance(v, bool) for v in weights):
        raise ValueError(f"{who}: weights must be {S} host numbers (one per scale), got {weights!r}")
    if not all(0.0 <= v < float("inf") for v in w) or not any(v > 0.0 for v in w):       # a NaN fails the comparison
        raise ValueError(f"{who}: weights={w} (finite, >= 0, not all zero)")
    return w


def knn_p(who: str, p, P: int) -> None:
    """The neighbours kept of a list of P: an integer (no bool), 1 <= p <= P."""
    if isinstance(p, bool) or not isinstance(p, numbers.Integral) or not 1 <= p <= P:      # numpy's integers are Integral, its bool_ is not
        raise ValueError(f"{who}: p={p!r} (an int, 1 .. P={P})")
