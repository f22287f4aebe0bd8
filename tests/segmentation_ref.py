"""CPU restatement of the PyanNet segmentation model (segmentation.py) that the GPU tests compare against.

It rounds where the kernels round (segmentation row) when `fmt` is "bf16" or "fp16", and nowhere when it is None:
  - weights, rounded once to the 2-byte format: the sinc filters (float64 -> fp32 -> 2-byte), conv, W_ih, W_hh, linear.0 and linear.1;
  - activation operands, split into two 2-byte planes (rnd2: hi = rnd(x), lo = rnd(x - hi); the MFMAs take hi and lo): the input of convs
    2 and 3, of every LSTM input projection, of every recurrence step (h_{t-1}) and of linear.0;
  - the head's first hidden layer, rounded once (one plane).
The tensors between stages (each SincNet block's output, every LSTM layer's output) are kept in fp32.  The samples enter exactly; the
waveform norm is the affine map a x + b (float64 statistics) applied after the conv as a conv(x) + b sum(w); c, the gates, the gate bias
b_ih + b_hh, the pooled maps and their norm statistics, the second hidden layer, the classifier and the log_softmax are unrounded.  `dtype` is the accumulation format: torch.float32 (the kernels' fp32 accumulation, in torch's order) or
torch.float64.
"""
from __future__ import annotations

import importlib
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as Fn

seg = importlib.import_module("speaker-diarization-toolkit_amd.segmentation")

PREC = {"bf16": 0, "fp16": 2}


def rnd(x: torch.Tensor, fmt: Optional[str]) -> torch.Tensor:
    """x rounded to the 2-byte format (fp16: saturated to +-65504, as the kernels store), in x's dtype."""
    if fmt is None:
        return x
    if fmt == "bf16":
        return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)
    return x.to(torch.float32).clamp(-65504, 65504).to(torch.float16).to(x.dtype)


def rnd2(x: torch.Tensor, fmt: Optional[str]) -> torch.Tensor:
    """x as the two-plane operand the kernels build from an fp32 value: hi = rnd(x), lo = rnd(x - hi), hi + lo."""
    if fmt is None:
        return x
    hi = rnd(x, fmt)
    return hi + rnd(x - hi, fmt)


def wround(a: np.ndarray, fmt: Optional[str], dtype) -> torch.Tensor:
    """A weight as the kernels hold it: fp32, then the 2-byte format."""
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32))
    return rnd(t, fmt).to(dtype)


class SegRef:
    def __init__(self, weights: Dict[str, np.ndarray], fmt: Optional[str] = "bf16", dtype=torch.float32):
        self.w, self.fmt, self.dtype = weights, fmt, dtype
        if fmt is None:
            f = torch.from_numpy(seg.sinc_filters(weights["sincnet.conv1d.0.filterbank.low_hz_"], weights["sincnet.conv1d.0.filterbank.band_hz_"]))
        else:
            f = torch.from_numpy(seg.rounded_sinc(weights, PREC[fmt]).astype(np.float64))
        self.sinc = f.to(dtype)
        self.sinc_sum = f.to(torch.float64).sum(1)

    def p(self, name: str) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(self.w[name], np.float32)).to(self.dtype)

    def W(self, name: str) -> torch.Tensor:
        return wround(self.w[name], self.fmt, self.dtype) if self.fmt else self.p(name)

    def _block(self, y, i):
        y = Fn.max_pool1d(y, 3, 3)
        mean = y.mean(2, keepdim=True)
        var = ((y - mean) ** 2).mean(2, keepdim=True)                 # biased; a single frame is served (var 0)
        y = (y - mean) / torch.sqrt(var + seg.NORM_EPS) * self.p(f"sincnet.norm1d.{i}.weight")[:, None] + self.p(f"sincnet.norm1d.{i}.bias")[:, None]
        return Fn.leaky_relu(y, 0.01)

    def frontend(self, pcm: np.ndarray) -> torch.Tensor:
        """pcm [B, S] int16 -> [B, F, 60] frames."""
        x = torch.from_numpy(pcm.astype(np.float64))
        mean = x.mean(1)
        var = ((x - mean[:, None]) ** 2).mean(1)
        a = float(self.w["sincnet.wav_norm1d.weight"][0]) / torch.sqrt(var + seg.NORM_EPS)
        b = float(self.w["sincnet.wav_norm1d.bias"][0]) - mean * a
        conv = Fn.conv1d(x.to(self.dtype)[:, None, :], self.sinc[:, None, :], stride=10)
        y = a.to(self.dtype)[:, None, None] * conv + (b[:, None, None] * self.sinc_sum[None, :, None]).to(self.dtype)
        y = self._block(torch.abs(y), 0)
        y = self._block(Fn.conv1d(rnd2(y, self.fmt), self.W("sincnet.conv1d.1.weight"), self.p("sincnet.conv1d.1.bias")), 1)
        y = self._block(Fn.conv1d(rnd2(y, self.fmt), self.W("sincnet.conv1d.2.weight"), self.p("sincnet.conv1d.2.bias")), 2)
        return y.transpose(1, 2).contiguous()

    def lstm_layer(self, l: int, x: torch.Tensor) -> torch.Tensor:
        """x [B, F, din] -> [B, F, 256] (forward | reverse)."""
        B, F, _ = x.shape
        outs = []
        for rev in (False, True):
            wi, wh, bi, bh = seg._lstm_names(l, rev)
            bias = (torch.from_numpy(self.w[bi].astype(np.float64)) + torch.from_numpy(self.w[bh].astype(np.float64)))
            if self.fmt is not None:
                bias = bias.to(torch.float32)                      # the packer's fp32 sum
            G = rnd2(x.to(self.dtype), self.fmt) @ self.W(wi).T + bias.to(self.dtype)
            Whh = self.W(wh)
            h = torch.zeros(B, 128, dtype=self.dtype)
            c = torch.zeros(B, 128, dtype=self.dtype)
            y = torch.empty(B, F, 128, dtype=self.dtype)
            for t in (range(F - 1, -1, -1) if rev else range(F)):
                gates = G[:, t] + rnd2(h, self.fmt) @ Whh.T
                i, f, g, o = gates.split(128, dim=1)
                c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
                h = torch.sigmoid(o) * torch.tanh(c)
                y[:, t] = h
            outs.append(y)
        return torch.cat(outs, dim=2)

    def head(self, x: torch.Tensor) -> torch.Tensor:
        h = rnd2(Fn.leaky_relu(rnd2(x, self.fmt) @ self.W("linear.0.weight").T + self.p("linear.0.bias"), 0.01), self.fmt)
        h = Fn.leaky_relu(h @ self.W("linear.1.weight").T + self.p("linear.1.bias"), 0.01)
        z = h @ self.p("classifier.weight").T + self.p("classifier.bias")
        return Fn.log_softmax(z, dim=-1)

    def forward(self, pcm: np.ndarray, keep: Optional[List] = None) -> torch.Tensor:
        """pcm [B, S] int16 -> logp [B, F, 7]; `keep` (a list) receives the input of every stage: frames, then each LSTM layer's output."""
        x = self.frontend(pcm)
        if keep is not None:
            keep.append(x)
        for l in range(4):
            x = self.lstm_layer(l, x)
            if keep is not None:
                keep.append(x)
        return self.head(x)


def mixed_audio(B, S, seed=0):
    """noise mixed with tone blocks and silence, int16"""
    rng = np.random.default_rng(seed)
    t = np.arange(S) / 16000.0
    x = np.zeros((B, S))
    for b in range(B):
        x[b] = rng.normal(0, 0.05 * (1 + b % 3), S)
        for _ in range(max(1, S // 16000)):
            a = int(rng.integers(0, max(1, S - 4000)))
            L = int(rng.integers(1000, 8000))
            x[b, a:a + L] += 0.3 * np.sin(2 * np.pi * rng.uniform(100, 3000) * t[a:a + L])
        s0 = int(rng.integers(0, S))
        x[b, s0:s0 + S // 8] = 0.0
    return np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16)


def stage_dims(S: int):
    """(L1, L2, F): the lengths after the sinc, conv-2 and conv-3 blocks (conv, then MaxPool1d(3, 3)) of a chunk of S samples."""
    L1 = ((S - 251) // 10 + 1) // 3
    L2 = (L1 - 4) // 3
    return L1, L2, (L2 - 4) // 3


def cut_windows(rec: np.ndarray, starts, S: int) -> np.ndarray:
    """The windows [s, s + S) of a 1-D int16 recording as rows [len(starts), S]; samples past the recording's end are zero."""
    rows = np.zeros((len(starts), S), np.int16)
    for i, s in enumerate(starts):
        piece = rec[int(s):int(s) + S]
        rows[i, :len(piece)] = piece
    return rows
