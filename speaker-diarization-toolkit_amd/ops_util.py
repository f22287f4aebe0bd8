"""What every module of host wrappers (ops.py and the ops_*.py mixins of Engine) shares: the pointer, stream and format helpers, and _need,
the device / dtype check of the identify path and of the building blocks (an SdkError; every other argument goes through _args.py)."""
from __future__ import annotations

from typing import Optional

import torch

from ._lib import SdkError


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _elem_fmt(t: torch.Tensor, what: str) -> int:
    """The C ABI's 2-byte element format of a tensor (the _fmt entry points' `precision`): bf16 -> 0, fp16 -> 2; any other dtype is refused."""
    if t.dtype == torch.bfloat16:
        return 0
    if t.dtype == torch.float16:
        return 2
    raise ValueError(f"{what}: 2-byte activations must be bfloat16 or float16, got {t.dtype}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise SdkError(f"{name} must live in device memory (got {t.device}); there is no CPU path")
    if t.dtype != dtype:
        raise SdkError(f"{name} must be {dtype}, got {t.dtype}")
    return t
