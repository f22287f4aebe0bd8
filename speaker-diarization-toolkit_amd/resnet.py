"""ResNet34 embedding extractor - the PyAnnote side of the upstream toolkit's "future backends" (speaker_detection_backends/backends.yaml:22-31):
PyAnnote 3.1's speaker embedding is the WeSpeaker ResNet34, a 2-D convolutional ResNet over the fbank image.  This is that PUBLIC architecture
(He et al. 2016 BasicBlocks, as WeSpeaker configures them for speaker verification) with base width 32:

  input     this build's 80-bin log-mel fbank [B*T, ldf], read as a one-channel image of height F = 80 (mel) and width T (frames)
  conv1     3x3, 1 -> 32, stride 1, zero padding 1, no bias; BN; ReLU
  layer1..4 BasicBlocks [3, 4, 6, 3], widths [32, 64, 128, 256], strides [1, 2, 2, 2] on the first block of each layer
            block: relu(bn2(conv2(relu(bn1(conv1(x))))) + shortcut(x)); both convs 3x3, padding 1, no bias; shortcut = 1x1 strided conv + BN
            where the stride or the width changes, else the identity.  Output sizes o = (n - 1) // 2 + 1: at T = 201, F x T goes
            80 x 201 -> 40 x 101 -> 20 x 51 -> 10 x 26
  pooling   temporal statistics of the final [256, 10, T'] map flattened in the public order (feature c * 10 + f, 2560 features): mean and
            std over t, std = sqrt(unbiased var + 1e-7) - WeSpeaker's TSTP as best known here (nothing on hand pins it; the choice is ours)
  seg_1     Linear 5120 -> embed_dim; its output is the embedding

Differences stated: the default embedding width is 192, not the public model's 256, because k3 / k4 / the .npy store are specialised to 192-d
(affinity_rowcol.hip dot192_*) - the x-vector family made the same choice.  PARITY UNPINNED: no checkpoint is available and none is fetched.
BN eps 1e-5.  Weights: fp32 host dict in the public state-dict naming - conv1.weight, bn1.{weight,bias,running_mean,running_var},
layer{i}.{j}.conv{1,2}.weight, layer{i}.{j}.bn{1,2}.*, layer{i}.0.shortcut.{0.weight,1.*}, seg_1.{weight,bias}; Backend reads them from
$SDK_RESNET_WEIGHTS (.npz in this naming).

Everything runs in libsdk_hip.so through ONE C call per batch (sdk_resnet_forward): sdk_resnet_conv2d per conv (an implicit GEMM over channel-last
maps; a downsampling block's projection shortcut is extra K columns of its conv2), the temporal statistics kernel, sdk_rows_fc.  Numerical
contracts: precision 0 (bf16 operands and layer-boundary storage) and 2 (one fp16 plane), with DESIGN section 3's layer-boundary rules - the
BN scale is folded into W in fp32 before the one rounding, every conv output is rounded once after its fp32 epilogue (bias, residual, ReLU),
pooling and seg_1 are fp32.  The precise mode (1) is not built for this family, and no bias correction is applied.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np

from . import _args
from .weights_pack import ALIGN, to_bits16

BN_EPS = 1e-5


@dataclass(frozen=True)
class ResNetConfig:
    n_feats: int = 80
    blocks: Tuple[int, ...] = (3, 4, 6, 3)
    widths: Tuple[int, ...] = (32, 64, 128, 256)
    embed_dim: int = 192

    def map_sizes(self, T: int) -> List[Tuple[int, int]]:
        """(F, T) of the stem's output and of every layer's output."""
        F, sizes = self.n_feats, [(self.n_feats, T)]
        for l in range(len(self.blocks)):
            if l:
                F, T = (F - 1) // 2 + 1, (T - 1) // 2 + 1
            sizes.append((F, T))
        return sizes

    def pooled_features(self) -> int:
        return 2 * self.widths[-1] * self.map_sizes(1)[-1][0]

    def param_count(self) -> int:
        return int(sum(int(np.prod(s)) for s in param_shapes(self).values()))

    def macs_per_segment(self, T: int) -> int:
        """Multiply-adds of one segment of T frames: every conv (the stem, both convs of every block, the projection shortcuts) and seg_1."""
        sizes = self.map_sizes(T)
        F, Tl = sizes[0]
        macs = F * Tl * self.widths[0] * 9
        cin = self.widths[0]
        for l, (nb, w) in enumerate(zip(self.blocks, self.widths)):
            Fo, To = sizes[l + 1]
            for j in range(nb):
                ci = cin if j == 0 else w
                macs += Fo * To * w * 9 * ci + Fo * To * w * 9 * w
                if j == 0 and (l > 0 or ci != w):
                    macs += Fo * To * w * ci
            cin = w
        return macs + self.pooled_features() * self.embed_dim


DEFAULT_RESNET = ResNetConfig()


class ResNetDesc(C.Structure):
    """sdk_resnet_desc (include/sdk_hip.h)."""
    _fields_ = [("n_feats", C.c_int32), ("embed_dim", C.c_int32), ("precision", C.c_int32), ("n_layers", C.c_int32),
                ("blocks", C.c_int32 * 4), ("width", C.c_int32 * 4), ("off", C.c_int64 * 72)]


def _has_projection(cfg: ResNetConfig, l: int, j: int) -> bool:
    cin = cfg.widths[l - 1] if l else cfg.widths[0]
    return j == 0 and (l > 0 or cin != cfg.widths[l])


def param_shapes(cfg: ResNetConfig = DEFAULT_RESNET) -> Dict[str, Tuple[int, ...]]:
    sh: Dict[str, Tuple[int, ...]] = {}

    def bn(name, c):
        for f in ("weight", "bias", "running_mean", "running_var"):
            sh[f"{name}.{f}"] = (c,)
    sh["conv1.weight"] = (cfg.widths[0], 1, 3, 3)
    bn("bn1", cfg.widths[0])
    cin = cfg.widths[0]
    for l, (nb, w) in enumerate(zip(cfg.blocks, cfg.widths)):
        for j in range(nb):
            p = f"layer{l + 1}.{j}"
            ci = cin if j == 0 else w
            sh[f"{p}.conv1.weight"] = (w, ci, 3, 3)
            bn(f"{p}.bn1", w)
            sh[f"{p}.conv2.weight"] = (w, w, 3, 3)
            bn(f"{p}.bn2", w)
            if _has_projection(cfg, l, j):
                sh[f"{p}.shortcut.0.weight"] = (w, ci, 1, 1)
                bn(f"{p}.shortcut.1", w)
        cin = w
    sh["seg_1.weight"] = (cfg.embed_dim, cfg.pooled_features())
    sh["seg_1.bias"] = (cfg.embed_dim,)
    return sh


def synthetic_weights(seed: int = 0, cfg: ResNetConfig = DEFAULT_RESNET) -> Dict[str, np.ndarray]:
    """Seeded He-scaled weights; BN statistics near identity (gamma in [0.8, 1.2], var in [0.5, 1.5]), except the residual branches' last BN
    (bn2: gamma in [0.3, 0.5]) - with identity shortcuts adding a full-gain branch in each of the 16 blocks, the activations' variance would double
    per block and the last maps leave the fp16 range."""
    rng = np.random.default_rng(seed)
    out: Dict[str, np.ndarray] = {}
    for name, shape in param_shapes(cfg).items():
        if name.endswith(".weight") and len(shape) >= 2:
            fan_in = int(np.prod(shape[1:]))
            gain = 1.0 if name.startswith("seg_1") else 2.0
            a = rng.standard_normal(shape, dtype=np.float32) * np.float32(np.sqrt(gain / fan_in))
        elif name.endswith("bn2.weight"):                                  # BN gamma of a residual branch
            a = rng.uniform(0.3, 0.5, shape).astype(np.float32)
        elif name.endswith(".weight"):                                     # BN gamma
            a = rng.uniform(0.8, 1.2, shape).astype(np.float32)
        elif name.endswith(".running_var"):
            a = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        else:                                                              # BN beta / running mean, seg_1 bias
            a = rng.standard_normal(shape, dtype=np.float32) * np.float32(0.1)
        out[name] = np.ascontiguousarray(a, dtype=np.float32)
    return out


def bn_fold(weights: Dict[str, np.ndarray], name: str) -> Tuple[np.ndarray, np.ndarray]:
    """Eval BN as (scale, shift) in float64."""
    g = weights[f"{name}.weight"].astype(np.float64)
    s = g / np.sqrt(weights[f"{name}.running_var"].astype(np.float64) + BN_EPS)
    return s, weights[f"{name}.bias"].astype(np.float64) - weights[f"{name}.running_mean"].astype(np.float64) * s


def tap_major(w: np.ndarray) -> np.ndarray:
    """[Cout, Cin, 3, 3] -> [Cout, 9 Cin], k = (3 dy + dx) Cin + c."""
    return np.ascontiguousarray(np.transpose(w, (0, 2, 3, 1)).reshape(w.shape[0], -1))


def folded_convs(weights: Dict[str, np.ndarray], cfg: ResNetConfig = DEFAULT_RESNET) -> List[Tuple[str, np.ndarray, np.ndarray]]:
    """The convs in launch order: (name, folded fp32 W [Cout, K], fp32 bias [Cout]).  The BN scale multiplies W in float64, rounded once to fp32;
    a downsampling block's conv2 carries its shortcut's folded 1x1 weights as the last Cin columns and the sum of both BN shifts as its bias."""
    out = []
    s, sh = bn_fold(weights, "bn1")
    out.append(("conv1", (weights["conv1.weight"].astype(np.float64).reshape(cfg.widths[0], 9) * s[:, None]).astype(np.float32), sh.astype(np.float32)))
    for l, nb in enumerate(cfg.blocks):
        for j in range(nb):
            p = f"layer{l + 1}.{j}"
            s1, b1 = bn_fold(weights, f"{p}.bn1")
            out.append((f"{p}.conv1", (tap_major(weights[f"{p}.conv1.weight"].astype(np.float64)) * s1[:, None]).astype(np.float32), b1.astype(np.float32)))
            s2, b2 = bn_fold(weights, f"{p}.bn2")
            w2 = tap_major(weights[f"{p}.conv2.weight"].astype(np.float64)) * s2[:, None]
            if f"{p}.shortcut.0.weight" in weights:
                ss, bs = bn_fold(weights, f"{p}.shortcut.1")
                wsc = weights[f"{p}.shortcut.0.weight"].astype(np.float64)[:, :, 0, 0] * ss[:, None]
                w2, b2 = np.concatenate([w2, wsc], axis=1), b2 + bs
            out.append((f"{p}.conv2", w2.astype(np.float32), b2.astype(np.float32)))
    return out


def pack_weights(weights: Dict[str, np.ndarray], precision: int = 0, cfg: ResNetConfig = DEFAULT_RESNET):
    """-> (blob uint8, ResNetDesc).  Slots (ALIGN-byte aligned): conv i at off[2 i] (2-byte bits of the folded W, [Cout, K] tap-major) and
    off[2 i + 1] (fp32 bias); seg_1 at off[66] (fp32 [features, embed_dim], transposed for sdk_rows_fc) and off[67] (fp32 bias).
    precision 0: bf16 bits; 2: fp16 bits (the features must then come from sdk_fbank_fmt(..., 2, ...)); 1 is refused."""
    if precision == 1:
        raise ValueError("SDK_PRECISION=1 (the precise mode) is not built for the ResNet34 family: use SDK_PRECISION=0 or 2")
    if precision not in (0, 2):
        raise ValueError(f"precision must be 0 or 2, got {precision}")
    if len(cfg.blocks) != 4 or cfg.widths[0] != 32 or any(w not in (32, 64, 128, 256) for w in cfg.widths):
        raise ValueError(f"the kernels serve 4 layers of widths in (32, 64, 128, 256) with a 32-wide stem, got {cfg.widths}")
    for k, s in param_shapes(cfg).items():
        if k not in weights or tuple(weights[k].shape) != s:
            raise ValueError(f"ResNet34 weight {k}: expected shape {s}, got {None if k not in weights else tuple(weights[k].shape)}")
    d = ResNetDesc()
    d.n_feats, d.embed_dim, d.precision, d.n_layers = cfg.n_feats, cfg.embed_dim, precision, 4
    for l in range(4):
        d.blocks[l], d.width[l] = cfg.blocks[l], cfg.widths[l]
    off = [-1] * 72
    chunks, cur = [], 0

    def put(slot, arr):
        nonlocal cur
        a = np.ascontiguousarray(arr)
        assert off[slot] == -1 and a.dtype in (np.uint16, np.float32)
        off[slot] = cur
        chunks.append((cur, a.view(np.uint8).reshape(-1)))
        cur += (a.nbytes + ALIGN - 1) // ALIGN * ALIGN

    for i, (_, w, b) in enumerate(folded_convs(weights, cfg)):
        put(2 * i, to_bits16(w, precision))
        put(2 * i + 1, b)
    put(66, np.ascontiguousarray(weights["seg_1.weight"].T, dtype=np.float32))
    put(67, weights["seg_1.bias"].astype(np.float32))
    d.off = (C.c_int64 * 72)(*off)
    blob = np.zeros(cur, np.uint8)
    for o, a in chunks:
        blob[o:o + a.size] = a
    return blob, d


class ResNet34:
    """Resident ResNet34 extractor on an ops.Engine (device blob + descriptor); embed_pcm mirrors Engine.embed_pcm and xvector.XVector.
    precision 0 (bf16) or 2 (one fp16 plane); the engine's front end is switched to that format by embed_pcm.  No bias correction."""

    def __init__(self, engine, weights: Dict[str, np.ndarray] = None, cfg: ResNetConfig = DEFAULT_RESNET, seed: int = 0, precision: int = 0):
        import torch
        self.eng, self.cfg, self.precision = engine, cfg, int(precision)
        self.weights = dict(weights if weights is not None else synthetic_weights(seed, cfg))
        self.bias_correction = False
        blob, self.desc = pack_weights(self.weights, self.precision, cfg)
        self.blob = torch.from_numpy(blob).to(engine.device)

    def effective_weights(self) -> Dict[str, np.ndarray]:
        return self.weights

    def forward(self, feats, B: int, T: int):
        """feats [B*T, ldf] as Engine.fbank writes them (bf16; precision 2: fp16) -> raw embeddings [B, embed_dim] fp32."""
        import torch
        from ._lib import check
        from .ops import _stream
        lib = self.eng.lib
        ws = self.eng._workspace("sdk_resnet_workspace_bytes", C.byref(self.desc), B, T, cache="resnet")
        emb = torch.empty((B, self.cfg.embed_dim), dtype=torch.float32, device=self.eng.device)
        check(lib.sdk_resnet_forward(self.eng.ctx, self.blob.data_ptr(), C.byref(self.desc), feats.data_ptr(), feats.stride(0), B, T,
                                     ws.data_ptr(), ws.numel(), emb.data_ptr(), _stream()), "sdk_resnet_forward")
        return emb

    def last_map_frames(self, T: int) -> int:
        """Width T4 of the last map for segments of T fbank frames (sdk_resnet_last_map_frames)."""
        return int(self.eng.lib.sdk_resnet_last_map_frames(C.byref(self.desc), int(T)))

    def forward_masked(self, feats, B: int, T: int, w, valid):
        """The forward with S weighted poolings per segment (sdk_resnet_forward_masked): the conv trunk runs once per segment, one pooling
        launch writes the S statistics rows.  w [B, S, T4] fp32 >= 0 and valid [B, S] int32 (device) -> raw embeddings [B * S, embed_dim]
        fp32, row b * S + s; rows with valid == 0 are zeros."""
        import torch
        from ._lib import check
        from .ops import _stream
        lib = self.eng.lib
        T4 = self.last_map_frames(T)
        S = int(_args.tensor("forward_masked", "w", w, "float32", (B, None, T4)).shape[1])      # T4: the width of the last map
        _args.tensor("forward_masked", "valid", valid, "int32", (B, S))
        ws = self.eng._workspace("sdk_resnet_masked_workspace_bytes", C.byref(self.desc), B, T, S, cache="resnet")
        emb = torch.empty((B * S, self.cfg.embed_dim), dtype=torch.float32, device=self.eng.device)
        check(lib.sdk_resnet_forward_masked(self.eng.ctx, self.blob.data_ptr(), C.byref(self.desc), feats.data_ptr(), feats.stride(0), B, T, S,
                                            w.data_ptr(), valid.data_ptr(), ws.data_ptr(), ws.numel(), emb.data_ptr(), _stream()),
              "sdk_resnet_forward_masked")
        return emb

    def embed_pcm(self, pcm):
        from .ops import num_frames
        B, S = pcm.shape
        if self.eng.precision != self.precision:
            self.eng.set_precision(self.precision)              # the front end's output format follows the numerical contract
        return self.eng.l2norm(self.forward(self.eng.fbank(pcm), B, num_frames(S)))
