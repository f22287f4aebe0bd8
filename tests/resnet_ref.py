"""CPU checker of the ResNet34 family (resnet.py): an independently composed torch.nn ResNet34 built from the public-name weight dict, and the
layer-boundary model of the GPU's numerical contract with explicit rounding sites.

Layer-boundary model (DESIGN section 3's rules): every BN is folded into its conv (scale into W in float64, then the folded W rounded once to the
storage format), every conv output is rounded once after its epilogue (bias, residual, ReLU) - the residual being the stored, rounded tensor -,
the pooling and seg_1 run un-rounded.  bits: 8 (bf16) or 11 (fp16, saturated at its finite range), with the packer's fp32 fold and fp32 biases;
None: no rounding site at all (folded weights and biases in float64) - the fp32 model.  The features are
taken as given: the caller rounds them to the storage format, as the front end does."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as Fn

EPS = 1e-5


def round_bits(x: torch.Tensor, bits: Optional[int]) -> torch.Tensor:
    if bits is None:
        return x
    if bits == 8:
        return x.to(torch.bfloat16).to(x.dtype)
    if bits == 11:
        return x.clamp(-65504.0, 65504.0).to(torch.float16).to(x.dtype)
    raise ValueError(f"bits={bits}: 8 (bf16), 11 (fp16) or None")


def _t(w: Dict[str, np.ndarray], k: str, dtype) -> torch.Tensor:
    return torch.from_numpy(np.asarray(w[k])).to(dtype)


class BasicBlock(torch.nn.Module):
    def __init__(self, cin: int, c: int, stride: int):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(cin, c, 3, stride, 1, bias=False)
        self.bn1 = torch.nn.BatchNorm2d(c, eps=EPS)
        self.conv2 = torch.nn.Conv2d(c, c, 3, 1, 1, bias=False)
        self.bn2 = torch.nn.BatchNorm2d(c, eps=EPS)
        self.shortcut = torch.nn.Sequential()
        if stride != 1 or cin != c:
            self.shortcut = torch.nn.Sequential(torch.nn.Conv2d(cin, c, 1, stride, bias=False), torch.nn.BatchNorm2d(c, eps=EPS))

    def forward(self, x):
        return torch.relu(self.bn2(self.conv2(torch.relu(self.bn1(self.conv1(x))))) + self.shortcut(x))


class ResNet34Module(torch.nn.Module):
    """The public WeSpeaker-style ResNet34 (base width 32) with temporal statistics pooling and seg_1; input feats [B, T, F]."""

    def __init__(self, n_feats=80, blocks=(3, 4, 6, 3), widths=(32, 64, 128, 256), embed_dim=192):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(1, widths[0], 3, 1, 1, bias=False)
        self.bn1 = torch.nn.BatchNorm2d(widths[0], eps=EPS)
        cin, f = widths[0], n_feats
        for l, (nb, w) in enumerate(zip(blocks, widths)):
            s = 1 if l == 0 else 2
            layer = [BasicBlock(cin, w, s)] + [BasicBlock(w, w, 1) for _ in range(nb - 1)]
            setattr(self, f"layer{l + 1}", torch.nn.Sequential(*layer))
            cin = w
            if l:
                f = (f - 1) // 2 + 1
        self.seg_1 = torch.nn.Linear(2 * widths[-1] * f, embed_dim)

    def forward(self, feats):
        x = feats.transpose(1, 2).unsqueeze(1)                            # [B, 1, F, T]
        x = torch.relu(self.bn1(self.conv1(x)))
        for l in range(1, 5):
            x = getattr(self, f"layer{l}")(x)
        x = x.reshape(x.shape[0], -1, x.shape[-1])                        # [B, C * F4, T4]: feature c * F4 + f
        stats = torch.cat([x.mean(dim=-1), torch.sqrt(x.var(dim=-1, unbiased=True) + 1e-7)], dim=1)
        return self.seg_1(stats)


def torch_resnet34(weights: Dict[str, np.ndarray], dtype=torch.float64, **cfg) -> ResNet34Module:
    m = ResNet34Module(**cfg).to(dtype).eval()
    sd = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in weights.items()}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    return m


def _fold(w, conv: str, bn: str, dtype):
    s = _t(w, f"{bn}.weight", torch.float64) / torch.sqrt(_t(w, f"{bn}.running_var", torch.float64) + EPS)
    shift = _t(w, f"{bn}.bias", torch.float64) - _t(w, f"{bn}.running_mean", torch.float64) * s
    return _t(w, f"{conv}.weight", torch.float64) * s[:, None, None, None], shift          # folded in float64


def layer_boundary_embed(weights: Dict[str, np.ndarray], feats: torch.Tensor, bits: Optional[int] = 8, blocks=(3, 4, 6, 3),
                         acc=torch.float64) -> torch.Tensor:
    """feats [B, T, F] (already in the storage format) -> raw embeddings [B, embed_dim] of the layer-boundary model."""
    def conv(x, conv_name, bn_name, stride, pad):                      # -> (conv output, float64 BN shift)
        wf, shift = _fold(weights, conv_name, bn_name, acc)
        if bits is not None:                                            # the packer's fp32 fold, then the storage rounding
            wf = round_bits(wf.to(torch.float32), bits)
        return Fn.conv2d(x, wf.to(acc), None, stride, pad), shift

    def f32(shift):                                                     # the fp32 bias the packer stores (no rounding site: float64)
        return shift.to(torch.float32).to(acc) if bits is not None else shift.to(acc)

    x = feats.to(acc).transpose(1, 2).unsqueeze(1)
    y, b = conv(x, "conv1", "bn1", 1, 1)
    x = round_bits(torch.relu(y + f32(b)[:, None, None]), bits)
    for l, nb in enumerate(blocks):
        for j in range(nb):
            p = f"layer{l + 1}.{j}"
            s = 2 if (j == 0 and l > 0) else 1
            y, b = conv(x, f"{p}.conv1", f"{p}.bn1", s, 1)
            h = round_bits(torch.relu(y + f32(b)[:, None, None]), bits)
            y, b = conv(h, f"{p}.conv2", f"{p}.bn2", 1, 1)
            if f"{p}.shortcut.0.weight" in weights:
                ys, bs = conv(x, f"{p}.shortcut.0", f"{p}.shortcut.1", s, 0)
                y, b = y + ys, b + bs                                  # one bias: both shifts summed in float64
                res = 0
            else:
                res = x
            x = round_bits(torch.relu(y + f32(b)[:, None, None] + res), bits)
    x = x.reshape(x.shape[0], -1, x.shape[-1])
    stats = torch.cat([x.mean(dim=-1), torch.sqrt(x.var(dim=-1, unbiased=True) + 1e-7)], dim=1)
    return stats @ _t(weights, "seg_1.weight", acc).T + _t(weights, "seg_1.bias", acc)


def conv_ref(x: torch.Tensor, wk: torch.Tensor, bias: torch.Tensor, stride: int, sc=None, wsc=None, sc_stride: int = 1, res=None, relu=True) -> torch.Tensor:
    """One sdk_resnet_conv2d in float64 on channel-last tensors: x [B, F, T, Cin], wk [Cout, 9 Cin] tap-major (k = (3 dy + dx) Cin + c),
    sc [B, Fsc, Tsc, Csc] with wsc [Cout, Csc], res [B, Fo, To, Cout] -> [B, Fo, To, Cout] before the storage rounding."""
    cout, cin = wk.shape[0], x.shape[-1]
    w = wk.double().reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)
    y = Fn.conv2d(x.double().permute(0, 3, 1, 2), w, None, stride, 1)
    if sc is not None:
        y = y + Fn.conv2d(sc.double().permute(0, 3, 1, 2), wsc.double()[:, :, None, None], None, sc_stride, 0)
    y = y.permute(0, 2, 3, 1) + bias.double()
    if res is not None:
        y = y + res.double()
    return torch.relu(y) if relu else y


def tstp_stats(x: torch.Tensor) -> torch.Tensor:
    """The temporal statistics pooling in float64 on the channel-last last map x [B, F, T, C] -> [B, 2 C F]: mean | sqrt(unbiased var + 1e-7)
    over t, feature c F + f."""
    x = x.double().permute(0, 3, 1, 2).reshape(x.shape[0], -1, x.shape[2])
    return torch.cat([x.mean(dim=-1), torch.sqrt(x.var(dim=-1, unbiased=True) + 1e-7)], dim=1)


def storage_ulp(v: torch.Tensor, bits: int) -> torch.Tensor:
    """Spacing of the 2-byte storage format (bits = 8: bf16, 11: fp16) at |v|; fp16 keeps its subnormal spacing 2^-24 below 2^-14."""
    _, e = torch.frexp(v.double().abs())
    u = torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - bits)
    u = torch.where(v == 0, torch.zeros_like(u), u)
    return u.clamp_min(2.0 ** -24) if bits == 11 else u
