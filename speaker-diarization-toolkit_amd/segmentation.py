"""PyanNet speaker segmentation - the third stage of PyAnnote 3.1's pipeline (next to its ResNet34 embedding, resnet.py, and its clustering,
cluster.agglomerative_cluster): per frame of a 10-s chunk, who of up to three local speakers is talking.  This is the PUBLIC architecture of
pyannote's segmentation-3.0 as best known here; nothing on hand pins it and no checkpoint is available or fetched, so PARITY IS UNPINNED.

  input      one chunk of S >= 991 samples, 16 kHz mono int16 (default S = 160 000: 10 s)
  wav norm   InstanceNorm1d(1, affine): per-chunk mean and biased variance over all S samples, eps 1e-5, then weight x^ + bias
  sinc       80 filters of 251 taps, stride 10, no padding, no bias: asteroid's ParamSincFB rule (as recalled from its public source),
             min_low_hz = min_band_hz = 50, built on the host in float64 from the 40 learnt low_hz_ / band_hz_ values:
               low = 50 + |low_hz_|,  high = clip(low + 50 + |band_hz_|, 50, 8000),  band = high - low
               n_ = 2 pi (-125 .. -1) / 16000,  window_ = 0.54 - 0.46 cos(2 pi linspace(0, 124.5, 125) / 251)
               cos filter f:  left = (sin(high n_) - sin(low n_)) / (n_ / 2) * window_,  [left, 2 band, flip(left)] / (2 band)   (filters 0..39)
               sin filter f:  left = (cos(low n_) - cos(high n_)) / (n_ / 2) * window_,  [left, 0, -flip(left)] / (2 band)     (filters 40..79)
             then |.|, MaxPool1d(3, 3), InstanceNorm1d(80, affine), LeakyReLU(0.01)
  conv 2     Conv1d(80, 60, 5), MaxPool1d(3, 3), InstanceNorm1d(60, affine), LeakyReLU
  conv 3     Conv1d(60, 60, 5), the same pool, norm and LeakyReLU
  frames     F(S) = ((((S - 251) // 10 + 1) // 3 - 4) // 3 - 4) // 3: F(160 000) = 589; frame i sees samples [270 i, 270 i + 991)
  lstm       nn.LSTM(60, 128, num_layers=4, bidirectional=True), gates i, f, g, o (dropout is training-only)
  head       Linear(256, 128) + LeakyReLU, Linear(128, 128) + LeakyReLU, Linear(128, 7), log_softmax
  powerset   classes {}, {0}, {1}, {2}, {0,1}, {0,2}, {1,2}: up to 3 local speakers, at most 2 active per frame

Weights: a host dict in pyannote's state-dict naming (param_shapes), loaded with from_public_state_dict (.npz through np.load without
pickle; the n_ / window_ buffers are ignored and rebuilt).  Everything runs in libsdk_hip.so (csrc/segmentation.hip) through one C call
per batch of chunks, sdk_segmentation_forward.  Numerical contract: precision 0 (bf16) or 2 (fp16) is the format of the
weights and of the MFMA operands; the int16 samples enter the sinc conv exactly and every activation operand enters as hi + lo planes of
that format split from fp32 (two MFMAs per product), the tensors between stages stay fp32.  The precise mode (1) is not built for this
family.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from .weights_pack import ALIGN, round16, to_bits16

SAMPLE_RATE = 16000
CHUNK = 160000
FRAME_HOP = 270                  # samples between frames
FRAME_FIRST = 495                # centre sample of frame 0
FRAME_SPAN = 991                 # samples a frame sees
POWERSET = ((), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2))
NORM_EPS = 1e-5

# slots of sdk_segmentation_desc.off (include/sdk_hip.h SDK_SEG_*)
SLOT_SINC, SLOT_SINC_SUM, SLOT_WAVNORM, SLOT_NORM0, SLOT_CONV1_W, SLOT_CONV1_B, SLOT_NORM1, SLOT_CONV2_W, SLOT_CONV2_B, SLOT_NORM2 = range(10)
SLOT_LSTM = 10
SLOT_LIN0_W, SLOT_LIN0_B, SLOT_LIN1_W, SLOT_LIN1_B, SLOT_CLS_W, SLOT_CLS_B = range(22, 28)
N_SLOTS = 28


@dataclass(frozen=True)
class SegmentationConfig:
    n_filters: int = 80
    sinc_taps: int = 251
    sinc_stride: int = 10
    min_low_hz: float = 50.0
    min_band_hz: float = 50.0
    conv_channels: int = 60
    conv_kernel: int = 5
    hidden: int = 128
    lstm_layers: int = 4
    linear: int = 128
    n_classes: int = 7

    def param_count(self) -> int:
        return int(sum(int(np.prod(s)) for s in param_shapes(self).values()))


DEFAULT_SEGMENTATION = SegmentationConfig()


def num_frames(S: int) -> int:
    """F(S): frames of a chunk of S samples (0 below 991)."""
    if S < FRAME_SPAN:
        return 0
    return ((((S - 251) // 10 + 1) // 3 - 4) // 3 - 4) // 3


def macs_per_chunk(S: int = CHUNK, cfg: SegmentationConfig = DEFAULT_SEGMENTATION) -> int:
    """Multiply-adds of one chunk: the sinc conv, convs 2 and 3, the LSTM input projections and recurrences (both directions), the head."""
    L0 = (S - cfg.sinc_taps) // cfg.sinc_stride + 1
    L1 = L0 // 3
    L2 = (L1 - 4) // 3
    F = num_frames(S)
    c, k, H = cfg.conv_channels, cfg.conv_kernel, cfg.hidden
    macs = L0 * cfg.n_filters * cfg.sinc_taps + (L1 - 4) * c * cfg.n_filters * k + (L2 - 4) * c * c * k
    for l in range(cfg.lstm_layers):
        din = c if l == 0 else 2 * H
        macs += 2 * F * 4 * H * (din + H)
    return macs + F * (2 * H * cfg.linear + cfg.linear * cfg.linear + cfg.linear * cfg.n_classes)


def recurrent_macs_per_chunk(S: int = CHUNK, cfg: SegmentationConfig = DEFAULT_SEGMENTATION) -> int:
    """The sequential part of macs_per_chunk: the W_hh products."""
    return cfg.lstm_layers * 2 * num_frames(S) * 4 * cfg.hidden * cfg.hidden


def _lstm_names(l: int, rev: bool) -> List[str]:
    sfx = f"_l{l}" + ("_reverse" if rev else "")
    return [f"lstm.weight_ih{sfx}", f"lstm.weight_hh{sfx}", f"lstm.bias_ih{sfx}", f"lstm.bias_hh{sfx}"]


def param_shapes(cfg: SegmentationConfig = DEFAULT_SEGMENTATION) -> Dict[str, Tuple[int, ...]]:
    nf, c, k, H = cfg.n_filters, cfg.conv_channels, cfg.conv_kernel, cfg.hidden
    sh: Dict[str, Tuple[int, ...]] = {
        "sincnet.wav_norm1d.weight": (1,), "sincnet.wav_norm1d.bias": (1,),
        "sincnet.conv1d.0.filterbank.low_hz_": (nf // 2, 1), "sincnet.conv1d.0.filterbank.band_hz_": (nf // 2, 1),
        "sincnet.conv1d.1.weight": (c, nf, k), "sincnet.conv1d.1.bias": (c,),
        "sincnet.conv1d.2.weight": (c, c, k), "sincnet.conv1d.2.bias": (c,),
        "sincnet.norm1d.0.weight": (nf,), "sincnet.norm1d.0.bias": (nf,),
        "sincnet.norm1d.1.weight": (c,), "sincnet.norm1d.1.bias": (c,),
        "sincnet.norm1d.2.weight": (c,), "sincnet.norm1d.2.bias": (c,),
    }
    for l in range(cfg.lstm_layers):
        din = c if l == 0 else 2 * H
        for rev in (False, True):
            wi, wh, bi, bh = _lstm_names(l, rev)
            sh[wi], sh[wh], sh[bi], sh[bh] = (4 * H, din), (4 * H, H), (4 * H,), (4 * H,)
    sh["linear.0.weight"], sh["linear.0.bias"] = (cfg.linear, 2 * H), (cfg.linear,)
    sh["linear.1.weight"], sh["linear.1.bias"] = (cfg.linear, cfg.linear), (cfg.linear,)
    sh["classifier.weight"], sh["classifier.bias"] = (cfg.n_classes, cfg.linear), (cfg.n_classes,)
    return sh


def sinc_filters(low_hz_: np.ndarray, band_hz_: np.ndarray, cfg: SegmentationConfig = DEFAULT_SEGMENTATION) -> np.ndarray:
    """The ParamSincFB rule of the module docstring in float64 -> [80, 251] (cosine filters 0..39, sine filters 40..79)."""
    K = cfg.sinc_taps
    low = cfg.min_low_hz + np.abs(np.asarray(low_hz_, np.float64).reshape(-1, 1))
    high = np.clip(low + cfg.min_band_hz + np.abs(np.asarray(band_hz_, np.float64).reshape(-1, 1)), cfg.min_low_hz, SAMPLE_RATE / 2)
    band = (high - low)[:, 0]
    n_lin = np.linspace(0, K / 2 - 1, int(K / 2))
    window = 0.54 - 0.46 * np.cos(2 * np.pi * n_lin / K)
    n_ = 2 * np.pi * np.arange(-(K - 1) / 2.0, 0).reshape(1, -1) / SAMPLE_RATE
    ft_low, ft_high = low @ n_, high @ n_
    left_c = (np.sin(ft_high) - np.sin(ft_low)) / (n_ / 2) * window
    left_s = (np.cos(ft_low) - np.cos(ft_high)) / (n_ / 2) * window
    cos_f = np.concatenate([left_c, 2 * band[:, None], left_c[:, ::-1]], axis=1) / (2 * band[:, None])
    sin_f = np.concatenate([left_s, np.zeros((len(band), 1)), -left_s[:, ::-1]], axis=1) / (2 * band[:, None])
    return np.concatenate([cos_f, sin_f], axis=0)


def _mel_init(cfg: SegmentationConfig) -> Tuple[np.ndarray, np.ndarray]:
    """asteroid's initial low_hz_ / band_hz_: 41 mel-spaced edges from 30 Hz to 8000 - (min_low + min_band) Hz."""
    to_mel = lambda hz: 2595 * np.log10(1 + hz / 700)          # noqa: E731
    to_hz = lambda mel: 700 * (10 ** (mel / 2595) - 1)          # noqa: E731
    hz = to_hz(np.linspace(to_mel(30.0), to_mel(SAMPLE_RATE / 2 - (cfg.min_low_hz + cfg.min_band_hz)), cfg.n_filters // 2 + 1))
    return hz[:-1].reshape(-1, 1), np.diff(hz).reshape(-1, 1)


def synthetic_weights(seed: int = 0, cfg: SegmentationConfig = DEFAULT_SEGMENTATION, lstm_gain: float = 3.5, recurrent_gain: float = 1.0,
                      classifier_gain: float = 20.0) -> Dict[str, np.ndarray]:
    """Seeded weights after PyTorch's default initialisation (U(-1/sqrt(fan_in), +) for convs and linears, U(-1/sqrt(128), +) for the LSTM),
    with W_ih at lstm_gain x, W_hh at recurrent_gain x and the classifier weights at classifier_gain x that scale, classifier bias 0: at the
    default init the head's output is nearly constant and one class wins every frame, and a larger W_hh makes the recurrence chaotic (its
    rounding spread grows faster than the argmax margins).  Norm weights in [0.8, 1.2], norm biases N(0, 0.1); the sinc band
    edges are asteroid's mel initialisation with a seeded +-10 % jitter."""
    rng = np.random.default_rng(seed)
    out: Dict[str, np.ndarray] = {}
    lo, bd = _mel_init(cfg)
    for name, shape in param_shapes(cfg).items():
        if name.endswith("low_hz_"):
            a = lo * rng.uniform(0.9, 1.1, shape)
        elif name.endswith("band_hz_"):
            a = bd * rng.uniform(0.9, 1.1, shape)
        elif "norm1d" in name:
            a = rng.uniform(0.8, 1.2, shape) if name.endswith("weight") else rng.normal(0, 0.1, shape)
        elif name.startswith("lstm."):
            bound = 1 / np.sqrt(cfg.hidden)
            a = rng.uniform(-bound, bound, shape) * (recurrent_gain if ".weight_hh" in name else lstm_gain if ".weight_ih" in name else 1.0)
        elif name == "classifier.bias":
            a = np.zeros(shape)
        else:                                                     # convs and linears
            wshape = param_shapes(cfg)[name.replace(".bias", ".weight")]
            bound = 1 / np.sqrt(int(np.prod(wshape[1:])))
            a = rng.uniform(-bound, bound, shape) * (classifier_gain if name == "classifier.weight" else 1.0)
        out[name] = np.ascontiguousarray(a, dtype=np.float32)
    return out


def from_public_state_dict(sd, prefix: str = "", cfg: SegmentationConfig = DEFAULT_SEGMENTATION) -> Dict[str, np.ndarray]:
    """A pyannote-named state dict (torch tensors or arrays; an optional key prefix such as "model." is stripped) -> the fp32 host dict.
    The sinc layer's n_ / window_ buffers are ignored (rebuilt by sinc_filters); every other missing or extra key, or a wrong shape, raises."""
    want = param_shapes(cfg)
    got: Dict[str, np.ndarray] = {}
    for k, v in sd.items():
        name = k[len(prefix):] if prefix and k.startswith(prefix) else k
        if name.endswith(".n_") or name.endswith(".window_"):
            continue
        if name not in want:
            raise ValueError(f"segmentation state dict: unexpected key {k!r}")
        a = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        if tuple(a.shape) != want[name]:
            raise ValueError(f"segmentation weight {name}: expected shape {want[name]}, got {tuple(a.shape)}")
        got[name] = np.ascontiguousarray(a, dtype=np.float32)
    missing = sorted(set(want) - set(got))
    if missing:
        raise ValueError(f"segmentation state dict: missing {missing[:4]}{' ...' if len(missing) > 4 else ''}")
    return got


def load_weights(path: str, prefix: str = "") -> Dict[str, np.ndarray]:
    """.npz in the public naming (np.load without pickle)."""
    with np.load(path, allow_pickle=False) as z:
        return from_public_state_dict({k: z[k] for k in z.files}, prefix)


class SegmentationDesc(C.Structure):
    """sdk_segmentation_desc (include/sdk_hip.h)."""
    _fields_ = [("precision", C.c_int32), ("reserved", C.c_int32), ("off", C.c_int64 * 32)]


def rounded_sinc(weights: Dict[str, np.ndarray], precision: int, cfg: SegmentationConfig = DEFAULT_SEGMENTATION) -> np.ndarray:
    """The sinc filters as the kernels use them: float64 -> fp32 -> the 2-byte format, as fp32 values [80, 251]."""
    f = sinc_filters(weights["sincnet.conv1d.0.filterbank.low_hz_"], weights["sincnet.conv1d.0.filterbank.band_hz_"], cfg)
    return round16(f.astype(np.float32), precision)


def pack_weights(weights: Dict[str, np.ndarray], precision: int = 0, cfg: SegmentationConfig = DEFAULT_SEGMENTATION):
    """-> (blob uint8, SegmentationDesc).  Slot layouts: include/sdk_hip.h SDK_SEG_*.  precision 0: bf16; 2: fp16; 1 is refused."""
    if precision == 1:
        raise ValueError("precision 1 (the precise mode) is not built for the segmentation model: use precision 0 (bf16) or 2 (fp16)")
    if precision not in (0, 2):
        raise ValueError(f"precision must be 0 or 2, got {precision}")
    if cfg != DEFAULT_SEGMENTATION:
        raise ValueError("the kernels serve the default PyanNet configuration only")
    for k, s in param_shapes(cfg).items():
        if k not in weights or tuple(np.shape(weights[k])) != s:
            raise ValueError(f"segmentation weight {k}: expected shape {s}, got {None if k not in weights else tuple(np.shape(weights[k]))}")
    w = {k: np.asarray(v, np.float32) for k, v in weights.items()}
    off = [-1] * 32
    chunks, cur = [], 0

    def put(slot, arr):
        nonlocal cur
        a = np.ascontiguousarray(arr)
        assert off[slot] == -1 and a.dtype in (np.uint16, np.float32)
        off[slot] = cur
        chunks.append((cur, a.view(np.uint8).reshape(-1)))
        cur += (a.nbytes + ALIGN - 1) // ALIGN * ALIGN

    def bits(a):
        return to_bits16(np.ascontiguousarray(a, np.float32), precision)

    sinc = np.zeros((80, 256), np.float32)
    sinc[:, :251] = sinc_filters(w["sincnet.conv1d.0.filterbank.low_hz_"], w["sincnet.conv1d.0.filterbank.band_hz_"], cfg).astype(np.float32)
    put(SLOT_SINC, bits(sinc))
    put(SLOT_SINC_SUM, round16(sinc, precision).astype(np.float64).sum(1).astype(np.float32))
    put(SLOT_WAVNORM, np.concatenate([w["sincnet.wav_norm1d.weight"], w["sincnet.wav_norm1d.bias"]]))
    for slot, i in ((SLOT_NORM0, 0), (SLOT_NORM1, 1), (SLOT_NORM2, 2)):
        put(slot, np.concatenate([w[f"sincnet.norm1d.{i}.weight"], w[f"sincnet.norm1d.{i}.bias"]]))
    c1 = np.zeros((64, 416), np.float32)                               # k = tap 80 + c
    c1[:60, :400] = np.transpose(w["sincnet.conv1d.1.weight"], (0, 2, 1)).reshape(60, 400)
    put(SLOT_CONV1_W, bits(c1))
    put(SLOT_CONV1_B, np.pad(w["sincnet.conv1d.1.bias"], (0, 4)))
    c2 = np.zeros((64, 5, 64), np.float32)                             # k = tap 64 + c
    c2[:60, :, :60] = np.transpose(w["sincnet.conv1d.2.weight"], (0, 2, 1))
    put(SLOT_CONV2_W, bits(c2.reshape(64, 320)))
    put(SLOT_CONV2_B, np.pad(w["sincnet.conv1d.2.bias"], (0, 4)))
    for l in range(4):
        kp = 64 if l == 0 else 256
        wih = np.zeros((1024, kp), np.float32)
        bias = np.zeros(1024, np.float32)
        whh = np.zeros((2, 512, 128), np.float32)
        for d, rev in enumerate((False, True)):
            wi, wh, bi, bh = _lstm_names(l, rev)
            wih[512 * d:512 * (d + 1), :w[wi].shape[1]] = w[wi]
            bias[512 * d:512 * (d + 1)] = (w[bi].astype(np.float64) + w[bh].astype(np.float64)).astype(np.float32)
            whh[d] = w[wh]
        put(SLOT_LSTM + 3 * l, bits(wih))
        put(SLOT_LSTM + 3 * l + 1, bias)
        put(SLOT_LSTM + 3 * l + 2, bits(whh))
    put(SLOT_LIN0_W, bits(w["linear.0.weight"]))
    put(SLOT_LIN0_B, w["linear.0.bias"])
    put(SLOT_LIN1_W, bits(w["linear.1.weight"]))
    put(SLOT_LIN1_B, w["linear.1.bias"])
    put(SLOT_CLS_W, w["classifier.weight"])
    put(SLOT_CLS_B, w["classifier.bias"])
    d = SegmentationDesc()
    d.precision = precision
    d.off = (C.c_int64 * 32)(*off)
    blob = np.zeros(cur, np.uint8)
    for o, a in chunks:
        blob[o:o + a.size] = a
    return blob, d


_POWERSET_MULTI = np.array([[k in cls for k in range(3)] for cls in POWERSET], dtype=bool)
_POWERSET_COUNT = np.array([len(cls) for cls in POWERSET], dtype=np.int64)


def powerset_to_multilabel(logp):
    """logp [..., 7] -> [..., 3] bool: the speakers of the argmax class (ties go to the lower class)."""
    import torch
    table = torch.as_tensor(_POWERSET_MULTI, device=logp.device)
    return table[torch.argmax(logp, dim=-1)]


def speaker_count(logp):
    """logp [..., 7] -> [...] int64: the number of active speakers of the argmax class."""
    import torch
    table = torch.as_tensor(_POWERSET_COUNT, device=logp.device)
    return table[torch.argmax(logp, dim=-1)]


class Segmentation:
    """Resident PyanNet on an ops.Engine (device blob + descriptor).  precision 0 (bf16) or 2 (one fp16 plane)."""

    def __init__(self, engine, weights: Optional[Dict[str, np.ndarray]] = None, precision: int = 0, seed: int = 0):
        import torch
        self.eng, self.precision = engine, int(precision)
        self.weights = dict(weights if weights is not None else synthetic_weights(seed))
        blob, self.desc = pack_weights(self.weights, self.precision)
        self.blob = torch.from_numpy(blob).to(engine.device)

    @staticmethod
    def _source(samples, starts, ld, B, S):
        """-> (samples, starts, ld, B, S, n): n samples are addressable from samples.data_ptr().  A [B, S] matrix may be a view with a row
        stride of its own (its extent is (B - 1) stride + S samples, not numel()); its samples must be contiguous within a row."""
        n = samples.numel()
        if starts is None:
            if samples.dim() == 2:
                if samples.shape[1] > 1 and samples.stride(1) != 1:
                    raise ValueError(f"segmentation: the samples of a row must be contiguous (stride(1)={samples.stride(1)})")
                B, S, ld = samples.shape[0], samples.shape[1], samples.stride(0)
                if B > 0:
                    n = (B - 1) * ld + S
            return samples, None, int(ld), int(B), int(S or CHUNK), int(n)
        return samples, starts, 0, int(starts.numel()), int(S or CHUNK), int(n)

    def forward(self, samples, starts=None, S: int = 0, ld: int = 0, B: int = 0):
        """samples: a [B, S] int16 device matrix (rows are chunks), or a 1-D recording with starts [B] int32 (device; chunks of S samples,
        default 160 000, are cut on the device, samples past the end read as zero) -> logp [B, F(S), 7] fp32 (device)."""
        import torch
        from ._lib import check
        from .ops import _stream
        samples, starts, ld, B, S, n = self._source(samples, starts, ld, B, S)
        lib = self.eng.lib
        F = num_frames(S)
        logp = torch.empty((B, max(F, 0), 7), dtype=torch.float32, device=self.eng.device)
        if B == 0:
            return logp
        ws = self.eng._workspace("sdk_segmentation_workspace_bytes", C.byref(self.desc), B, S, cache="segmentation")
        check(lib.sdk_segmentation_forward(self.eng.ctx, self.blob.data_ptr(), C.byref(self.desc), samples.data_ptr(), n,
                                           starts.data_ptr() if starts is not None else None, ld, B, S, ws.data_ptr(), ws.numel(),
                                           logp.data_ptr(), _stream()), "sdk_segmentation_forward")
        return logp

    def frontend(self, samples, starts=None, S: int = 0, ld: int = 0, B: int = 0):
        """The SincNet stages alone -> [B F, 64] fp32 frames (features 0..59, 60..63 zero)."""
        import torch
        from ._lib import check
        from .ops import _stream
        samples, starts, ld, B, S, n = self._source(samples, starts, ld, B, S)
        lib = self.eng.lib
        out = torch.empty((B * num_frames(S), 64), dtype=torch.float32, device=self.eng.device)
        if B == 0:
            return out
        ws = self.eng._workspace("sdk_segmentation_workspace_bytes", C.byref(self.desc), B, S, cache="segmentation")
        check(lib.sdk_sincnet_frontend(self.eng.ctx, self.blob.data_ptr(), C.byref(self.desc), samples.data_ptr(), n,
                                       starts.data_ptr() if starts is not None else None, ld, B, S, ws.data_ptr(), ws.numel(),
                                       out.data_ptr(), _stream()), "sdk_sincnet_frontend")
        return out

    def bilstm_layer(self, layer: int, x, B: int, F: int):
        """One BiLSTM layer: x [B F, ld] fp32 (layer 0: 60 features, ld >= 64; else 256) -> [B F, 256] fp32 (forward | reverse)."""
        import torch
        from ._lib import check
        from .ops import _stream
        y = torch.empty((B * F, 256), dtype=torch.float32, device=self.eng.device)
        ws = self.eng._scratch_bytes("segmentation_lstm", B * F * 4096)             # (no sizer: the gate pre-activations, [B F][1024] fp32)
        check(self.eng.lib.sdk_bilstm_layer(self.eng.ctx, self.blob.data_ptr(), C.byref(self.desc), int(layer), x.data_ptr(), x.stride(0), B, F,
                                            ws.data_ptr(), ws.numel(), y.data_ptr(), _stream()), "sdk_bilstm_layer")
        return y


# ---------------------------------------------------------------------------------------------------- aggregation (Backend.speech_ranges)
def chunk_starts(n_samples: int, step_s: float = 1.0, chunk: int = CHUNK) -> np.ndarray:
    """First samples of the chunks: 0, step, 2 step, ... while a chunk fits; then one chunk ending at the recording's end.  A recording
    shorter than a chunk is one chunk (zero-padded)."""
    hop = int(round(step_s * SAMPLE_RATE))
    if hop <= 0:
        raise ValueError(f"step_s={step_s}: must be positive")
    if n_samples <= chunk:
        return np.zeros(1, np.int64)
    st = np.arange(0, n_samples - chunk + 1, hop, dtype=np.int64)
    if st[-1] + chunk < n_samples:
        st = np.append(st, n_samples - chunk)
    return st


def aggregate_counts(counts: np.ndarray, starts: np.ndarray, n_samples: int):
    """Per-chunk speaker counts [C, F] (chunks first at starts [C]) -> (speech, overlap): lists of (start_s, end_s).
    Global frame g (centre 270 g + 495; g = 0 .. G - 1, the frames whose centre lies inside the recording) takes frame
    i = floor((270 g - start_c + 135) / 270) of chunk c (round half up) when 0 <= i < F.  It is speech when the mean of [count >= 1] over its
    contributing chunks is at least 0.5, overlap when the mean of [count >= 2] is.  A run of frames g0 .. g1 is the range
    [(270 g0 + 360) / 16000, (270 g1 + 630) / 16000)."""
    counts = np.asarray(counts)
    Cn, F = counts.shape
    G = max(0, (n_samples - FRAME_FIRST + FRAME_HOP - 1) // FRAME_HOP)
    sp, ov, nc = np.zeros(G), np.zeros(G), np.zeros(G)
    for c in range(Cn):
        q = (135 - int(starts[c])) // FRAME_HOP                        # i = g + q
        g = np.arange(F) - q
        m = (g >= 0) & (g < G)
        np.add.at(sp, g[m], counts[c][m] >= 1)
        np.add.at(ov, g[m], counts[c][m] >= 2)
        np.add.at(nc, g[m], 1)
    has = nc > 0
    speech = has & (2 * sp >= nc)
    overlap = has & (2 * ov >= nc)
    return frames_to_ranges(speech), frames_to_ranges(overlap)


def frames_to_ranges(active: np.ndarray) -> List[Tuple[float, float]]:
    out = []
    g, n = 0, len(active)
    while g < n:
        if active[g]:
            g1 = g
            while g1 + 1 < n and active[g1 + 1]:
                g1 += 1
            out.append(((FRAME_HOP * g + 360) / SAMPLE_RATE, (FRAME_HOP * g1 + 630) / SAMPLE_RATE))
            g = g1 + 1
        else:
            g += 1
    return out
