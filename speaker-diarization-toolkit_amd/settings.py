"""The Backend's environment variables that are read at call time, one reader each: a plain function that parses its variable in the one
way backend.py always has, whenever it is called - nothing is cached, so a variable changed on a live Backend is followed (the enrolled
vectors' numerical setting and the batch size rely on it).  backend.py's docstring is the user-facing reference of what each variable
means.  The decision-rule variables (SDK_COHORT*, SDK_SCORE_*) belong to rules.rule_from_env; SDK_MODEL, SDK_DIARIZE_MODEL, SDK_WINDOW_S and
SDK_HOP_S are read once, by Backend.__init__."""
from __future__ import annotations

import os
from typing import Optional, Tuple


def device() -> int:
    """SDK_DEVICE: the GPU index (default: $LOCAL_RANK, else 0)."""
    return int(os.environ.get("SDK_DEVICE", os.environ.get("LOCAL_RANK", "0")))


def precision_text() -> Optional[str]:
    """SDK_PRECISION as it was written (None: not set), for a refusal that quotes it."""
    return os.environ.get("SDK_PRECISION")


def precision() -> int:
    """SDK_PRECISION: 0 (bf16, the default), 1 (the precise mode) or 2 (one fp16 plane)."""
    return int(os.environ.get("SDK_PRECISION", "0"))


def max_batch() -> int:
    """SDK_MAX_BATCH: the windows of one forward batch (default 2048, at least 1)."""
    return max(1, int(os.environ.get("SDK_MAX_BATCH", "2048")))


def segmentation_batch() -> int:
    """SDK_SEGMENTATION_BATCH: the chunks of one segmentation batch (default 256, at least 1)."""
    return max(1, int(os.environ.get("SDK_SEGMENTATION_BATCH", "256")))


def lite() -> bool:
    """SDK_NO_TORCH=1: the torch-free host path."""
    return os.environ.get("SDK_NO_TORCH") == "1"


def bias_correction() -> bool:
    """SDK_BIAS_CORRECTION: on unless it is "0"."""
    return os.environ.get("SDK_BIAS_CORRECTION", "1") != "0"


def weights_path(variable: str) -> Optional[str]:
    """The checkpoint a weights variable names (SDK_ECAPA_WEIGHTS, SDK_XVECTOR_WEIGHTS, SDK_RESNET_WEIGHTS, SDK_SEGMENTATION_WEIGHTS);
    None or empty: the seeded synthetic weights."""
    return os.environ.get(variable)


def ecapa_layout() -> str:
    """SDK_ECAPA_LAYOUT: "public" for a checkpoint in the public state-dict naming, anything else for the .npz naming of weights.py."""
    return os.environ.get("SDK_ECAPA_LAYOUT", "native")


def ecapa_prefix() -> str:
    """SDK_ECAPA_PREFIX: the key prefix stripped from a public checkpoint."""
    return os.environ.get("SDK_ECAPA_PREFIX", "")


def cache_build_timeout_s() -> float:
    """SDK_CACHE_BUILD_TIMEOUT_S: how long the torch-free path waits for the child process that fills the packed-weight cache."""
    return float(os.environ.get("SDK_CACHE_BUILD_TIMEOUT_S", "300"))


def diarizer_plda() -> Optional[Tuple[str, str, int]]:
    """The PLDA model of the diarizer's embedding space: (SDK_PLDA_TRANSFORM, SDK_PLDA, SDK_PLDA_DIM: 64 or 128, default 128), or None when
    neither file is named.  One file without the other is refused."""
    tpath, ppath = os.environ.get("SDK_PLDA_TRANSFORM"), os.environ.get("SDK_PLDA")
    if bool(tpath) != bool(ppath):
        raise ValueError("SDK_PLDA_TRANSFORM and SDK_PLDA name the two files of one PLDA model: set both or neither")
    if not tpath:
        return None
    dim = os.environ.get("SDK_PLDA_DIM", "128")
    if dim not in ("64", "128"):
        raise ValueError(f"SDK_PLDA_DIM={dim!r}: the PLDA dimensions kept, 64 or 128")
    return tpath, ppath, int(dim)
