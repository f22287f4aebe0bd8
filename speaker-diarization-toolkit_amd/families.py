"""The embedding families SDK_MODEL selects, one row each: everything the Backend needs to know about a family is a field of its row,
so a further family is one more row.  The rows import their model modules (weights, xvector, resnet) only when a field that needs one is
used: importing this module, like importing backend, stays cheap and leaves torch out."""
from __future__ import annotations

import importlib
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Tuple

import numpy as np

from . import settings


def load_npz_weights(path, check: Callable[[Dict[str, np.ndarray]], object]) -> Dict[str, np.ndarray]:
    """An .npz checkpoint as a dict of contiguous fp32 arrays (numpy's non-executing loader), passed through the family's shape check,
    which raises a ValueError that names the tensor."""
    with np.load(path, allow_pickle=False) as z:
        weights = {k: np.ascontiguousarray(z[k], dtype=np.float32) for k in z.files}
    check(weights)
    return weights


def _load_ecapa(path) -> Dict[str, np.ndarray]:
    """SDK_ECAPA_LAYOUT=public: a checkpoint in the public ECAPA-TDNN state-dict naming (weights.from_public_state_dict); default: the
    .npz naming of weights.py.  Both through non-executing loaders only."""
    from . import weights
    if settings.ecapa_layout() == "public":
        return weights.load_public_checkpoint(path, prefix=settings.ecapa_prefix())
    return load_npz_weights(path, weights.check_weights)


@dataclass(frozen=True)
class Family:
    name: str                                   # the value of SDK_MODEL
    weights_env: str                            # the variable that names its checkpoint
    label: str                                  # how messages call it
    module: str                                 # the submodule with its default config, synthetic_weights and shape check
    config_name: str                            # its default config there
    tag: str                                    # its part of model_version, formatted with c = the config
    check_name: str                             # the shape check there: raises a ValueError that names the tensor
    extractor_name: Optional[str]               # its extractor class there, built on an engine; None: the engine's own forward
    cached: bool                                # whether its packed blob is kept in the on-disk cache (weights_cache.py)
    bias_correction: bool                       # whether SDK_BIAS_CORRECTION applies to it
    precisions: Tuple[int, ...]                 # the SDK_PRECISION values it serves
    lite: bool                                  # whether the torch-free host path (SDK_NO_TORCH=1) serves it
    load_checkpoint: Optional[Callable] = None  # path -> weights; None: load_npz_weights with its shape check
    lite_load: Optional[Callable] = None        # (lite.LiteEngine, weights) -> None; None: the engine's own cached blob

    def _module(self):
        return importlib.import_module(f"{__package__}.{self.module}")

    @property
    def config(self):
        return getattr(self._module(), self.config_name)

    @property
    def embed_dim(self) -> int:
        return self.config.embed_dim

    @property
    def version_tag(self) -> str:
        return self.tag.format(c=self.config)

    @property
    def check(self) -> Callable[[Dict[str, np.ndarray]], object]:
        return getattr(self._module(), self.check_name)

    def load(self, path) -> Dict[str, np.ndarray]:
        return self.load_checkpoint(path) if self.load_checkpoint is not None else load_npz_weights(path, self.check)

    def synthetic(self) -> Dict[str, np.ndarray]:
        return self._module().synthetic_weights(0)

    def host_weights(self) -> Dict[str, np.ndarray]:
        """The checkpoint its variable names, else the seeded synthetic weights."""
        path = settings.weights_path(self.weights_env)
        return self.load(path) if path else self.synthetic()

    def extractor(self, engine, weights, precision: int):
        """Its resident extractor on an ops.Engine (the bias correction: $SDK_BIAS_CORRECTION, where it applies)."""
        return getattr(self._module(), self.extractor_name)(engine, weights, precision=precision)


FAMILIES: Dict[str, Family] = {f.name: f for f in (
    Family("ecapa", "SDK_ECAPA_WEIGHTS", "ECAPA-TDNN", "weights", "DEFAULT_CONFIG", "ecapa1024", "check_weights", None,
           cached=True, bias_correction=True, precisions=(0, 1, 2), lite=True, load_checkpoint=_load_ecapa),
    Family("xvector", "SDK_XVECTOR_WEIGHTS", "x-vector", "xvector", "DEFAULT_XVECTOR", "xvector{c.channels[0]}", "pack_weights", "XVector",
           cached=False, bias_correction=True, precisions=(0, 1, 2), lite=True, lite_load=lambda eng, weights: eng.load_xvector(weights)),
    # 4.4 M / 6.3 M parameters (x-vector / ResNet34): packed in well under a second, not cached
    Family("resnet34", "SDK_RESNET_WEIGHTS", "ResNet34", "resnet", "DEFAULT_RESNET", "resnet34", "pack_weights", "ResNet34",
           cached=False, bias_correction=False, precisions=(0, 2), lite=False),
)}
