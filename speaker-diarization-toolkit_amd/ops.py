"""Host-side wrappers over the C ABI: torch tensors in, torch tensors out, every byte of compute
inside libsdk_hip.so.  torch supplies device memory and the current HIP stream only.

`Engine` is the long-lived per-process, per-GPU object (context + resident weights + fbank
tables + reusable scratch): the reference constructs its backend once per CLI process
(speaker_detection_backends/base.py:291-293), so everything expensive lives here and is built
lazily exactly once.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib, resample
from ._lib import ConvGemmArgs, EcapaDesc, SdkError, check
from .weights import DEFAULT_CONFIG, EcapaConfig, synthetic_weights
from .weights_pack import N_MELS_PADDED, N_MELS_PADDED_HP, pack_weights

HOP = 160
EMBED_DIM = 192


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


THIN_MAX = 32      # KV of csrc/spectral.hip: the widest [n, k] block (and the most centres) the thin helpers take


def _thin(t, name: str, what: str, shape=None, dtype=torch.float32, contiguous: bool = True) -> torch.Tensor:
    """An argument of a thin [n, k] helper (rows_gram ... kmeans_assign), which the kernels read through a bare pointer as a contiguous
    array of `dtype`: anything else is refused here, before any launch, with a ValueError that names the argument.  shape: the exact
    shape it must have (None = not checked); contiguous=False where the caller passes t.contiguous() on."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise ValueError(f"{what}: {name} must live in device memory (got {t.device}); there is no CPU path")
    if t.dtype != dtype:
        raise ValueError(f"{what}: {name} must be {dtype}, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} must have shape {list(shape)}, got {list(t.shape)}")
    if contiguous and not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous, got shape {list(t.shape)} with strides {list(t.stride())} (pass {name}.contiguous())")
    return t


def _thin_rows(X, name: str, what: str):
    """The [n, k] row block of a thin helper: 2-D, n >= 1, 1 <= k <= THIN_MAX, fp32, contiguous -> (n, k)."""
    _thin(X, name, what, contiguous=False)
    if X.dim() != 2 or X.shape[0] < 1:
        raise ValueError(f"{what}: {name} must be [n, k] with n >= 1, got {list(X.shape)}")
    if not 1 <= X.shape[1] <= THIN_MAX:
        raise ValueError(f"{what}: k = {X.shape[1]} (the width of {name}) must be in 1..{THIN_MAX}")
    _thin(X, name, what)
    return int(X.shape[0]), int(X.shape[1])


def num_frames(n_samples: int) -> int:
    return 1 + n_samples // HOP


STREAM_RING = 1024       # SDK_STREAM_RING: frames a stream's ring holds, and the most a step emits


class StreamState:
    """Engine.stream_state: the opaque device block of a bank of live streams (buf) and the rows its steps write."""

    def __init__(self, eng, R: int, capacity: int, d: int, nbytes: int):
        dev = eng.device
        self.R, self.capacity, self.d, self.nbytes = R, capacity, d, nbytes
        self.buf = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self.labels = torch.full((R, 3), -1, dtype=torch.int32, device=dev)
        self.score = torch.zeros((R, 3), dtype=torch.float32, device=dev)
        self.K = torch.zeros((R,), dtype=torch.int32, device=dev)
        self.emit_lo = torch.zeros((R,), dtype=torch.int64, device=dev)
        self.emit_n = torch.zeros((R,), dtype=torch.int32, device=dev)
        self.count = torch.zeros((R, STREAM_RING), dtype=torch.uint8, device=dev)
        self.speakers = torch.full((R, STREAM_RING, 2), -1, dtype=torch.int32, device=dev)


class Engine:
    def __init__(self, device: int = 0, weights: Optional[Dict[str, np.ndarray]] = None,
                 cfg: EcapaConfig = DEFAULT_CONFIG, seed: int = 0, cache_key: Optional[str] = None, weights_fn=None, digest_fn=None,
                 bias_correction: Optional[bool] = None):
        """weights: host dict (weights.py naming) or None; weights_fn: called only when the dict is really needed (cache miss);
        cache_key / digest_fn: identity of the weights for the packed-blob cache (weights_cache.py) - None = no caching.
        bias_correction (default mode only): fold the constant part of the bf16 weight-rounding error of every GEMM layer into its bias,
        from a calibration pass on built-in synthetic audio (weights_pack.bias_corrections; PCM -> score deviation from the fp32 model
        4.3e-3 -> ~8e-4 at no run-time cost).  False = the plain bf16 layer-boundary model (kernel parity tests).  None = $SDK_BIAS_CORRECTION
        (default "1")."""
        self.lib = _lib.load_library()
        self.ctx = _lib.get_ctx(device)        # raises SdkError without a gfx950 device
        self.device = torch.device("cuda", device)
        self.cfg = cfg
        self._weights_host = weights
        self._weights_fn = weights_fn
        self._cache_key = cache_key
        self._digest_fn = digest_fn
        self.cache_hit = False
        import os
        self.bias_correction = (os.environ.get("SDK_BIAS_CORRECTION", "1") != "0") if bias_correction is None else bool(bias_correction)
        self._bias_host: Dict[str, np.ndarray] = {}        # layer name -> corrected bias of the CURRENT single-plane mode, for effective_weights()
        self._bias_by_precision: Dict[int, Dict[str, np.ndarray]] = {}
        self._seed = seed
        self._wblob = None
        self._desc = None
        self._packed = {}                 # precision -> (device blob, desc): each numerical contract has its own weight format
        self.precision = 0
        self._fbank_tabs = None
        self._scratch: Dict[str, torch.Tensor] = {}
        self._graphs: Dict[tuple, tuple] = {}
        self._streams = []
        self._taps: Dict[tuple, torch.Tensor] = {}
        self._ingest = None

    # ------------------------------------------------------------------ resident state
    def _scratch_bytes(self, key: str, nbytes: int) -> torch.Tensor:
        key = f"{key}@{torch.cuda.current_stream().cuda_stream}"       # scratch is per stream: sub-batches overlap
        buf = self._scratch.get(key)
        if buf is None or buf.numel() < nbytes:
            self._scratch[key] = buf = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
        return buf

    def fbank_tables(self) -> torch.Tensor:
        if self._fbank_tabs is None:
            n = self.lib.sdk_fbank_tables_bytes()
            host = np.zeros(n, dtype=np.uint8)
            check(self.lib.sdk_fbank_tables_fill(host.ctypes.data, n), "sdk_fbank_tables_fill")
            self._fbank_tabs = torch.from_numpy(host).to(self.device)
        return self._fbank_tabs

    def load_weights(self, weights: Optional[Dict[str, np.ndarray]] = None) -> None:
        if weights is not None:
            self._weights_host = weights
            self._packed.clear()
            self._cache_key = None                      # explicit weights: their identity is unknown to the cache
        if self.precision not in self._packed:
            from . import weights_cache
            correct = self.bias_correction and self.precision in (0, 2)
            from .weights_pack import calibration_tag
            ckey = (f"{self.precision}c" + calibration_tag()) if correct else self.precision   # a bias-corrected blob is its own cache entry (per calibration recording)
            hit = weights_cache.load_blob(self._cache_key, ckey) if self._cache_key else None
            need_store = False
            if hit is not None:
                blob, f = hit                            # memory-mapped: the upload below is the only pass over the bytes
                self.cache_hit = True
            else:
                if self._weights_host is None:
                    self._weights_host = self._weights_fn() if self._weights_fn else synthetic_weights(self._seed, self.cfg)
                blob, f = pack_weights(self._weights_host, self.cfg, precision=self.precision)
                need_store = bool(self._cache_key and self._digest_fn)
            d = EcapaDesc()
            for k, v in f.items():
                if k == "dilation":
                    d.dilation = (C.c_int32 * 4)(*v)
                elif k == "off":
                    d.off = (C.c_int64 * 256)(*v)
                else:
                    setattr(d, k, v)
            import warnings
            with warnings.catch_warnings():          # a cache hit is a read-only memory map: it is only read (uploaded) here
                warnings.simplefilter("ignore", UserWarning)
                host = torch.from_numpy(np.asarray(blob))
            self._packed[self.precision] = (host.to(self.device), d)
            if correct and hit is None:
                blob = self._apply_bias_correction(np.array(blob, copy=True), f)
            if need_store:
                weights_cache.store(self._cache_key, self._digest_fn(), ckey, blob, f)
        self._wblob, self._desc = self._packed[self.precision]

    # ------------------------------------------------------------------ bias correction of the bf16 weight rounding (default mode)
    @staticmethod
    def calibration_pcm(n: int = 24, seed: int = 20240) -> np.ndarray:
        """Built-in calibration audio (weights_pack.calibration_pcm: torch-free, shared with the lite host path)."""
        from .weights_pack import calibration_pcm
        return calibration_pcm(n, seed)

    def _apply_bias_correction(self, blob: np.ndarray, fields: dict) -> np.ndarray:
        """One calibration forward with the plain blob (already uploaded), corrected biases computed on the host from the measured channel means of
        every GEMM layer's input, written into the device blob and into `blob` (returned, for the cache)."""
        from .weights_pack import bias_corrections, bias_slot, calib_layout
        wdev, d = self._packed[self.precision]
        pcm = torch.from_numpy(self.calibration_pcm()).to(self.device)
        B, S = pcm.shape
        T = num_frames(S)
        saved = (self._wblob, self._desc)
        self._wblob, self._desc = wdev, d
        try:
            feats = self.fbank(pcm)
            nfl = self.lib.sdk_ecapa_calib_floats(C.byref(d), B)
            calib = torch.zeros((nfl,), dtype=torch.float32, device=self.device)
            ws = self._scratch_bytes("ecapa", self.lib.sdk_ecapa_workspace_bytes(C.byref(d), B, T))
            emb = torch.empty((B, self.cfg.embed_dim), dtype=torch.float32, device=self.device)
            check(self.lib.sdk_ecapa_forward_calib(self.ctx, wdev.data_ptr(), C.byref(d), feats.data_ptr(), feats.stride(0), B, T, ws.data_ptr(),
                                                   ws.numel(), emb.data_ptr(), calib.data_ptr(), _stream()), "sdk_ecapa_forward_calib")
            cal = calib.cpu().numpy().astype(np.float64)
        finally:
            self._wblob, self._desc = saved
        layout, per_seg = calib_layout(self.cfg)
        assert per_seg * B == nfl, (per_seg, B, nfl)
        means = {name: cal[off * B:(off + 2 * ch) * B].reshape(B, 2 * ch)[:, :ch].mean(axis=0) for name, ch, off in layout}
        self._bias_by_precision[self.precision] = self._bias_host = bias_corrections(self._weights_host, means, self.cfg, precision=self.precision)
        for name, bias in self._bias_host.items():
            o = fields["off"][bias_slot(name, self.cfg)]
            raw = np.ascontiguousarray(bias, dtype=np.float32).view(np.uint8)
            blob[o:o + raw.size] = raw
            wdev[o:o + raw.size] = torch.from_numpy(raw.copy()).to(self.device)
        return blob

    def effective_weights(self) -> Dict[str, np.ndarray]:
        """The weight dictionary whose bf16 layer-boundary model the default mode computes: the loaded weights with the corrected biases
        (identical to the loaded weights when bias_correction is off).  For checkers (tests, smoke): the product never needs it."""
        self.desc
        if self._weights_host is None:
            self._weights_host = self._weights_fn() if self._weights_fn else synthetic_weights(self._seed, self.cfg)
        w = dict(self._weights_host)
        if self.bias_correction and self.precision in (0, 2):
            self._bias_host = self._bias_by_precision.setdefault(self.precision, {})
            if not self._bias_host:                   # cache hit: read the corrected biases back from the device blob
                from .weights_pack import bias_slot, calib_layout
                for name, ch, _ in calib_layout(self.cfg)[0]:
                    n_out = self._weights_host[f"{name}.conv.b"].shape[0]
                    o = int(self._desc.off[bias_slot(name, self.cfg)])
                    self._bias_host[name] = self._wblob[o:o + 4 * n_out].cpu().numpy().view(np.float32).copy()
            for name, b in self._bias_host.items():
                w[f"{name}.conv.b"] = b
        return w

    def set_precision(self, precision: int) -> None:
        """0 (default): bf16 GEMM operands, bf16 layer-boundary storage - PCM -> cosine score within ~4e-3 of the fp32 model.
        1: the precise mode (csrc/hp.hip): fp16 hi+lo planes and three MFMAs per product everywhere, within 1e-5 (north_star's
        tolerance), ~3x the GEMM time.  Selects the fbank output format and the weight blob together; embeddings of the two modes
        are comparable with each other at the 4e-3 level only.
        2 (round 5): one fp16 plane - the default mode's kernels and schedule with fp16 instead of bf16 storage and MFMA operands (11
        significand bits instead of 8): PCM -> score within ~1e-4 of the fp32 model with the bias correction, at the default mode's MFMA
        count (the chip holds a ~5 % lower clock on fp16 products: profiles/r05_gemm_f16_probe.txt)."""
        if precision not in (0, 1, 2):
            raise SdkError(f"precision must be 0, 1 or 2, got {precision}")
        self.precision = precision          # (every call names its format: the library context holds no per-engine state)
        self._wblob = self._desc = None
        self._graphs.clear()

    @property
    def desc(self) -> EcapaDesc:
        if self._desc is None:
            self.load_weights()
        return self._desc

    def debug_ptr(self, name: str, tensor: Optional[torch.Tensor]) -> None:
        """Diagnostics: hand a device buffer to (or, with None, take it away from) an in-kernel probe (sdk_debug_set_ptr)."""
        check(self.lib.sdk_debug_set_ptr(self.ctx, name.encode(), tensor.data_ptr() if tensor is not None else None), "sdk_debug_set_ptr")

    def set_option(self, name: str, value: int) -> None:
        check(self.lib.sdk_set_option(self.ctx, name.encode(), int(value)), "sdk_set_option")

    # ------------------------------------------------------------------ measurement
    def profile_begin(self) -> None:
        check(self.lib.sdk_profile_begin(self.ctx), "sdk_profile_begin")

    def profile_end(self) -> Dict[str, Dict[str, float]]:
        """Per kernel family: launches, summed device ms (HIP events on the launch stream), flops, bytes."""
        rep = _lib.ProfileReport()
        check(self.lib.sdk_profile_end(self.ctx, C.byref(rep)), "sdk_profile_end")
        return {name: {"launches": rep.launches[i], "ms": rep.ms[i], "flops": rep.flops[i], "bytes": rep.bytes[i]}
                for i, name in enumerate(_lib.KERNEL_FAMILIES) if rep.launches[i]}

    # ------------------------------------------------------------------ audio conversion
    def resample_s16(self, x: torch.Tensor, rate_in: int, rate_out: int = 16000) -> torch.Tensor:
        """x int16 [n] or [n, C] interleaved (device) at rate_in -> mono int16 [ceil(n*L/M)] at rate_out."""
        _need(x, torch.int16, "x")
        x = x.contiguous()
        n_in = x.shape[0]
        ch = 1 if x.dim() == 1 else x.shape[1]
        taps, L, M, K = resample.design_taps(int(rate_in), int(rate_out))
        key = (int(rate_in), int(rate_out))
        tdev = self._taps.get(key)
        if tdev is None:
            tdev = self._taps[key] = torch.from_numpy(np.array(taps)).to(self.device)
        n_out = resample.out_len(n_in, L, M)
        y = torch.empty((n_out,), dtype=torch.int16, device=self.device)
        check(self.lib.sdk_resample_s16(self.ctx, x.data_ptr(), n_in, ch, tdev.data_ptr(), L, M, K, y.data_ptr(), n_out, _stream()),
              "sdk_resample_s16")
        return y

    def resample_s16_host(self, x: np.ndarray, rate_in: int, rate_out: int = 16000) -> np.ndarray:
        """Host arrays in and out (wav.decode_to_profile; lite.LiteEngine has the same method)."""
        return self.resample_s16(torch.from_numpy(np.ascontiguousarray(x)).to(self.device), rate_in, rate_out).cpu().numpy()

    # ------------------------------------------------------------------ k1
    def fbank(self, pcm: torch.Tensor, ldf: Optional[int] = None) -> torch.Tensor:
        """pcm [B, S] int16 (device) -> feats [B*T, ldf] bf16 (channels >= 80 are zero); in precise mode fp16 planes
        [B*T, 2 x 96]: hi values in columns [0, 96), lo values (times 2^11) in [96, 192)."""
        _need(pcm, torch.int16, "pcm")
        pcm = pcm.contiguous()
        B, S = pcm.shape
        T = num_frames(S)
        if ldf is None:
            ldf = 2 * N_MELS_PADDED_HP if self.precision == 1 else N_MELS_PADDED
        feats = torch.empty((B * T, ldf), dtype=torch.bfloat16 if self.precision == 0 else torch.float16, device=self.device)
        wsb = self.lib.sdk_fbank_workspace_bytes(B, S)
        ws = self._scratch_bytes("fbank", wsb)
        check(self.lib.sdk_fbank_fmt(self.ctx, pcm.data_ptr(), B, S, self.fbank_tables().data_ptr(), feats.data_ptr(), ldf,
                                     ws.data_ptr(), ws.numel(), self.precision, _stream()), "sdk_fbank")
        return feats

    def fbank_windows(self, samples_ptr: int, n_samples: int, starts_ptr: int, B: int, S: int, ldf: Optional[int] = None) -> torch.Tensor:
        """fbank with the windows cut on the device (sdk_fbank_windows): samples_ptr -> int16 [n_samples] resident recording, starts_ptr -> int32 [B]
        first samples; same features as fbank() on the materialised [B, S] windows, bit for bit."""
        T = num_frames(S)
        if ldf is None:
            ldf = 2 * N_MELS_PADDED_HP if self.precision == 1 else N_MELS_PADDED
        feats = torch.empty((B * T, ldf), dtype=torch.bfloat16 if self.precision == 0 else torch.float16, device=self.device)
        ws = self._scratch_bytes("fbank", self.lib.sdk_fbank_workspace_bytes(B, S))
        check(self.lib.sdk_fbank_windows_fmt(self.ctx, samples_ptr, n_samples, starts_ptr, B, S, self.fbank_tables().data_ptr(), feats.data_ptr(), ldf,
                                             ws.data_ptr(), ws.numel(), self.precision, _stream()), "sdk_fbank_windows")
        return feats

    def ingest(self):
        """The staging runtime (ingest.py / csrc/ingest.hip): pinned, double-buffered, on a copy stream of its own."""
        if self._ingest is None:
            from .ingest import Ingest
            self._ingest = Ingest(self.lib, self.ctx, depth=2)
        return self._ingest

    def embed_from_host(self, samples: np.ndarray, tables: Dict[int, np.ndarray], step: int = 2048, forward=None):
        """One recording in HOST memory (int16 [n]) + window-start tables {window samples S: int32 [B_S]} -> {S: (E, Eb, resid)} device tensors.
        The recording is uploaded once through the pinned staging slots (the next call's upload overlaps this call's forward); the overlapping
        windows are never materialised.  Windows go through in batches of `step`; forward(feats, B, T) defaults to the ECAPA-TDNN forward
        (Backend passes the x-vector's).  Bit-identical to embed_pcm on the host-cut windows."""
        from .ingest import chunk_samples, plan_chunks
        forward = forward or self.ecapa_forward
        self.desc if forward == self.ecapa_forward else None          # lazy weight load (its uploads run on the current stream) before the fan-out
        st = _stream()
        ing = self.ingest()
        samples = np.ascontiguousarray(samples, dtype=np.int16).reshape(-1)
        pieces = plan_chunks(len(samples), tables, chunk_samples())   # one piece unless the recording is longer than a staging slot may be
        out: Dict[int, tuple] = {}
        for lo, hi, sub in pieces:
            order = sorted(sub)
            flat = np.concatenate([sub[S][1] for S in order]) if order else np.zeros((0,), np.int32)
            ticket, ds, dw = ing.submit(samples[lo:hi], flat, max(order) if order else 0, st)      # piece i + 1 uploads under piece i's forward
            off = 0
            try:
                for S in order:
                    rows, local = sub[S]
                    Bs = len(local)
                    if Bs == 0:                                        # an empty table: its (empty) result is made below
                        continue
                    parts = []
                    for a in range(0, Bs, step):
                        b = min(step, Bs - a)
                        feats = self.fbank_windows(ds, hi - lo, dw + 4 * (off + a), b, S)
                        parts.append(self.l2norm(forward(feats, b, num_frames(S))))
                    res = parts[0] if len(parts) == 1 else tuple(torch.cat([p[i] for p in parts], dim=0) for i in range(3))
                    if rows is None:
                        out[S] = res
                    else:                                              # scatter this piece's windows to their rows of the table
                        if S not in out:
                            out[S] = tuple(torch.empty((len(tables[S]),) + tuple(r.shape[1:]), dtype=r.dtype, device=r.device) for r in res)
                        ridx = torch.from_numpy(rows).to(self.device)
                        for dst, r in zip(out[S], res):
                            dst[ridx] = r
                    off += Bs
            finally:
                ing.release(ticket, st)
            self.last_ingest_ticket = ticket
        for S in tables:                                               # an empty table still has an (empty) result
            if S not in out:
                out[S] = (torch.empty((0, self.cfg.embed_dim), dtype=torch.float32, device=self.device),
                          torch.empty((0, self.cfg.embed_dim), dtype=torch.bfloat16, device=self.device), torch.empty((0,), dtype=torch.float32, device=self.device))
        return out

    # ------------------------------------------------------------------ k2
    def ecapa_forward(self, feats: torch.Tensor, B: int, T: int) -> torch.Tensor:
        """feats [B*T, ldf] bf16 (precise mode: fp16 planes) -> raw embeddings [B, 192] fp32."""
        _need(feats, torch.bfloat16 if self.precision == 0 else torch.float16, "feats")
        if feats.shape[0] != B * T or feats.stride(1) != 1:
            raise SdkError(f"feats must be [B*T={B * T}, ldf] row-major, got {tuple(feats.shape)}")
        d = self.desc
        wsb = self.lib.sdk_ecapa_workspace_bytes(C.byref(d), B, T)
        ws = self._scratch_bytes("ecapa", wsb)
        emb = torch.empty((B, self.cfg.embed_dim), dtype=torch.float32, device=self.device)
        check(self.lib.sdk_ecapa_forward(self.ctx, self._wblob.data_ptr(), C.byref(d), feats.data_ptr(), feats.stride(0),
                                         B, T, ws.data_ptr(), ws.numel(), emb.data_ptr(), _stream()), "sdk_ecapa_forward")
        return emb

    def ecapa_forward_masked(self, feats: torch.Tensor, B: int, T: int, w: torch.Tensor, valid: torch.Tensor) -> torch.Tensor:
        """The ECAPA-TDNN forward with S masked attentive statistics poolings per chunk (sdk_ecapa_forward_masked; the rule is in
        include/sdk_hip.h): the trunk runs once per chunk, bit for bit ecapa_forward's; w [B, S, T] fp32 >= 0 (any weights) and valid [B, S]
        int32, both on the device -> raw embeddings [B * S, embed_dim] fp32, row b * S + s; rows with valid == 0, or without weight, are
        zeros.  Precision 0 and 2 (the precise mode is refused)."""
        if self.precision == 1:
            raise SdkError("ecapa_forward_masked: precision 1 (the precise mode) is not built for the masked pooling: use precision 0 or 2")
        _need(feats, torch.bfloat16 if self.precision == 0 else torch.float16, "feats")
        if feats.shape[0] != B * T or feats.stride(1) != 1:
            raise SdkError(f"feats must be [B*T={B * T}, ldf] row-major, got {tuple(feats.shape)}")
        if not isinstance(w, torch.Tensor) or w.dim() != 3 or w.shape[0] != B or w.shape[2] != T or w.dtype != torch.float32 or not w.is_contiguous() or not w.is_cuda:
            raise ValueError(f"ecapa_forward_masked: w must be a contiguous fp32 device tensor [B = {B}, S, T = {T}], got "
                             f"{tuple(w.shape) if isinstance(w, torch.Tensor) else type(w).__name__} {getattr(w, 'dtype', None)}")
        S = int(w.shape[1])
        if not 1 <= S <= 8:
            raise ValueError(f"ecapa_forward_masked: S = {S} weight rows per chunk (served: 1 .. 8)")
        if not isinstance(valid, torch.Tensor) or tuple(valid.shape) != (B, S) or valid.dtype != torch.int32 or not valid.is_contiguous() or not valid.is_cuda:
            raise ValueError(f"ecapa_forward_masked: valid must be a contiguous int32 device tensor [{B}, {S}], got "
                             f"{tuple(valid.shape) if isinstance(valid, torch.Tensor) else type(valid).__name__} {getattr(valid, 'dtype', None)}")
        d = self.desc
        ws = self._scratch_bytes("ecapa_masked", self.lib.sdk_ecapa_masked_workspace_bytes(C.byref(d), B, T, S))
        emb = torch.empty((B * S, self.cfg.embed_dim), dtype=torch.float32, device=self.device)
        check(self.lib.sdk_ecapa_forward_masked(self.ctx, self._wblob.data_ptr(), C.byref(d), feats.data_ptr(), feats.stride(0), B, T, S,
                                                w.data_ptr(), valid.data_ptr(), ws.data_ptr(), ws.numel(), emb.data_ptr(), _stream()),
              "sdk_ecapa_forward_masked")
        return emb

    # ------------------------------------------------------------------ k3
    def l2norm(self, X: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """X [N, d] fp32 -> (E fp32 unit rows, Eb bf16 copy, resid [N] = ||E - Eb||)."""
        _need(X, torch.float32, "X")
        X = X.contiguous()
        N, d = X.shape
        E = torch.empty_like(X)
        Eb = torch.empty((N, d), dtype=torch.bfloat16, device=self.device)
        r = torch.empty((N,), dtype=torch.float32, device=self.device)
        check(self.lib.sdk_l2norm(self.ctx, X.data_ptr(), N, d, E.data_ptr(), Eb.data_ptr(), r.data_ptr(), _stream()), "sdk_l2norm")
        return E, Eb, r

    # ------------------------------------------------------------------ k4
    def affinity_topk(self, E, Eb, re, P, Pb, rp_max, k: int = 1, want_count: bool = False):
        """Cosine affinity of unit rows E [N,192] vs P [Pn,192] -> (idx [N,k] int32, score [N,k] fp32).
        rp_max: device tensor [1] = max profile residual (from l2norm)."""
        for t, dt, nm in ((E, torch.float32, "E"), (Eb, torch.bfloat16, "Eb"), (re, torch.float32, "resid_e"),
                          (P, torch.float32, "P"), (Pb, torch.bfloat16, "Pb"), (rp_max, torch.float32, "resid_p")):
            _need(t, dt, nm)
        N, d = E.shape
        Pn = P.shape[0]
        idx = torch.empty((N, k), dtype=torch.int32, device=self.device)
        sc = torch.empty((N, k), dtype=torch.float32, device=self.device)
        cnt = torch.zeros((1,), dtype=torch.int32, device=self.device) if want_count else None
        ws = self._scratch_bytes("affinity", self.lib.sdk_affinity_workspace_bytes(N, Pn))
        check(self.lib.sdk_affinity_topk(self.ctx, E.data_ptr(), Eb.data_ptr(), re.data_ptr(), P.data_ptr(), Pb.data_ptr(),
                                         rp_max.data_ptr(), N, Pn, d, k, idx.data_ptr(), sc.data_ptr(), _ptr(cnt),
                                         ws.data_ptr(), ws.numel(), _stream()), "sdk_affinity_topk")
        return (idx, sc, cnt) if want_count else (idx, sc)

    # ------------------------------------------------------------------ adaptive score normalisation (snorm.py)
    @staticmethod
    def _snorm_rows(name: str, what: str, t, d: Optional[int] = None) -> Tuple[int, int]:
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"{name}: {what} must be a contiguous fp32 [rows, d] device tensor, got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__} {getattr(t, 'dtype', '')}")
        n, dd = int(t.shape[0]), int(t.shape[1])
        if dd < 64 or dd > 512 or dd % 64:
            raise ValueError(f"{name}: d={dd} not supported (a multiple of 64, at most 512)")
        if d is not None and dd != d:
            raise ValueError(f"{name}: {what} has d={dd}, expected {d}")
        return n, dd

    @staticmethod
    def _snorm_vec(name: str, what: str, t, n: int) -> None:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (n,) or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"{name}: {what} must be a contiguous fp32 [{n}] device tensor, got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__} {getattr(t, 'dtype', '')}")

    def cohort_stats(self, E: torch.Tensor, cohort: torch.Tensor, K: int, ws: Optional[torch.Tensor] = None):
        """Unit fp32 rows E [N, d] and cohort [M, d] (device) -> (mean [N], std [N]) fp32 of every row's K largest cohort cosines: the mean and
        the population standard deviation, floored at snorm.STD_FLOOR (sdk_cohort_stats).  ws: a uint8 device tensor to use as the workspace
        (default: one of sdk_cohort_stats_workspace_bytes(N, M, K) bytes is allocated)."""
        N, d = self._snorm_rows("cohort_stats", "E", E)
        M, _ = self._snorm_rows("cohort_stats", "the cohort", cohort, d)
        K = int(K)
        if M < 1 or M > (1 << 20):
            raise ValueError(f"cohort_stats: M={M} cohort rows (1 .. 2^20)")
        if K < 1 or K > M:
            raise ValueError(f"cohort_stats: K={K} (1 .. M={M})")
        nbytes = int(self.lib.sdk_cohort_stats_workspace_bytes(N, M, K))
        if nbytes == 0:
            raise SdkError(f"sdk_cohort_stats_workspace_bytes: {self.lib.sdk_last_error().decode()}")
        if ws is None:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=E.device)
        elif ws.dtype != torch.uint8 or ws.dim() != 1 or not ws.is_cuda or not ws.is_contiguous():
            raise ValueError(f"cohort_stats: ws must be a contiguous uint8 device tensor, got {tuple(ws.shape)} {ws.dtype}")
        mean = torch.empty((N,), dtype=torch.float32, device=E.device)
        std = torch.empty((N,), dtype=torch.float32, device=E.device)
        check(self.lib.sdk_cohort_stats(self.ctx, E.data_ptr(), N, cohort.data_ptr(), M, d, K, mean.data_ptr(), std.data_ptr(), ws.data_ptr(),
                                        ws.numel(), _stream()), "sdk_cohort_stats")
        return mean, std

    def affinity_topk_snorm(self, E: torch.Tensor, mean_e: torch.Tensor, std_e: torch.Tensor, P: torch.Tensor, mean_p: torch.Tensor,
                            std_p: torch.Tensor, k: int = 1):
        """Unit fp32 rows E [N, d] and P [Pn, d] with their cohort statistics (cohort_stats) -> (idx [N, k] int32, score [N, k] fp32,
        raw [N, k] fp32): per window the k <= min(4, Pn) largest z = ((s - mean_e) / std_e + (s - mean_p) / std_p) / 2, s the cosine; ties to
        the lower profile; raw is s.  A slot without a finite z holds (-1, 0, 0) (sdk_affinity_topk_snorm)."""
        N, d = self._snorm_rows("affinity_topk_snorm", "E", E)
        Pn, _ = self._snorm_rows("affinity_topk_snorm", "P", P, d)
        self._snorm_vec("affinity_topk_snorm", "mean_e", mean_e, N)
        self._snorm_vec("affinity_topk_snorm", "std_e", std_e, N)
        self._snorm_vec("affinity_topk_snorm", "mean_p", mean_p, Pn)
        self._snorm_vec("affinity_topk_snorm", "std_p", std_p, Pn)
        k = int(k)
        if k < 1 or k > 4:
            raise ValueError(f"affinity_topk_snorm: k={k} (1 .. 4)")
        if Pn < 1 or k > Pn:
            raise ValueError(f"affinity_topk_snorm: k={k} with Pn={Pn} profiles (the caller clamps k to the number of profiles, at least 1)")
        idx = torch.empty((N, k), dtype=torch.int32, device=E.device)
        sc = torch.empty((N, k), dtype=torch.float32, device=E.device)
        raw = torch.empty((N, k), dtype=torch.float32, device=E.device)
        check(self.lib.sdk_affinity_topk_snorm(self.ctx, E.data_ptr(), mean_e.data_ptr(), std_e.data_ptr(), N, P.data_ptr(), mean_p.data_ptr(),
                                               std_p.data_ptr(), Pn, d, k, idx.data_ptr(), sc.data_ptr(), raw.data_ptr(), _stream()),
              "sdk_affinity_topk_snorm")
        return idx, sc, raw

    # ------------------------------------------------------------------ whole path
    def embed_pcm(self, pcm: torch.Tensor):
        """pcm [B, S] int16 on device -> (E, Eb, resid) L2-normalised embeddings."""
        B, S = pcm.shape
        feats = self.fbank(pcm)
        emb = self.ecapa_forward(feats, B, num_frames(S))
        return self.l2norm(emb)

    def embed_pcm_overlapped(self, pcm: torch.Tensor, nsplit: int = 2):
        """embed_pcm with the batch cut into `nsplit` sub-batches, each on its own HIP stream.  Segments are
        independent, so the sub-batches need no ordering between them; the dispatcher co-schedules the
        HBM-bound sweeps (SE, pooling, fbank) of one sub-batch into the wave slots, registers and LDS the
        MFMA-bound GEMMs of the other leave free on every CU, and one sub-batch's tail overlaps the other's head."""
        B = pcm.shape[0]
        if nsplit <= 1 or B < 2 * nsplit:
            return self.embed_pcm(pcm)
        # lazy state first, on THIS stream and complete: the weight upload, the calibration pass and the 29 bias patches of a first load must not
        # race with the side streams that read the same blob
        self.desc
        self.fbank_tables()
        torch.cuda.current_stream().synchronize()
        if len(self._streams) < nsplit:
            self._streams += [torch.cuda.Stream(device=self.device) for _ in range(nsplit - len(self._streams))]
        cur = torch.cuda.current_stream()
        parts = []
        for i, chunk in enumerate(pcm.chunk(nsplit)):
            st = self._streams[i]
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                parts.append(self.embed_pcm(chunk))
        for i in range(len(parts)):
            cur.wait_stream(self._streams[i])
        E = torch.cat([p[0] for p in parts]); Eb = torch.cat([p[1] for p in parts]); r = torch.cat([p[2] for p in parts])
        for t in (E, Eb, r):
            t.record_stream(cur)
        return E, Eb, r

    def embed_pcm_graph(self, pcm: torch.Tensor):
        """embed_pcm replayed from a captured HIP graph (one graph per input shape): ~45 launches become one
        submission, which is what bounds the latency of a single-recording identify (B <= ~64 windows).
        The returned tensors are the graph's static outputs - consume them before the next call."""
        key = tuple(pcm.shape)
        entry = self._graphs.get(key)
        if entry is None:
            static_in = pcm.clone()
            self.embed_pcm(static_in)                    # warm-up: lazy state (weights, tables, scratch, function attributes)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = self.embed_pcm(static_in)
            entry = self._graphs[key] = (graph, static_in, out)
        graph, static_in, out = entry
        static_in.copy_(pcm)
        graph.replay()
        return out

    # ------------------------------------------------------------------ building blocks (tests / tuning)
    def conv_gemm(self, A, W, N, Cin, taps=1, dil=1, T=None, bias=None, scale=None, shift=None, ubias=None,
                  relu=False, tanh=False, out_bf16=True, out_f32=False, X2=None, stats_mode=0, A2=None, tap_pack=0,
                  a_kblocked=False, c_kblocked=False):
        """stats_mode 1/2 additionally returns the fused per-segment column statistics as a 4th value
        ([B, N] means, or [B, 2N] mean | std).
        a_kblocked: A is a K-blocked tensor [Cin / 64, M, 64] (to_kblocked); c_kblocked: the bf16 output comes back as [N / 64, M, 64]
        (include/sdk_hip.h SDK_GEMM_A_KBLOCKED / SDK_GEMM_C_KBLOCKED)."""
        _need(A, torch.bfloat16, "A"); _need(W, torch.bfloat16, "W")
        if a_kblocked and (A.dim() != 3 or A.shape[2] != 64 or A.shape[0] * 64 != Cin or not A.is_contiguous()):
            raise ValueError(f"conv_gemm: a K-blocked A must be a contiguous [Cin / 64, M, 64] tensor, got {tuple(A.shape)} for Cin={Cin}")
        M = A.shape[1] if a_kblocked else A.shape[0]
        T = T or M
        g = ConvGemmArgs()
        g.A, g.lda, g.W = A.data_ptr(), (64 if a_kblocked else A.stride(0)), W.data_ptr()
        if A2 is not None:
            g.A2, g.lda2 = A2.data_ptr(), A2.stride(0)
        Cout = torch.empty((N // 64, M, 64) if c_kblocked else (M, N), dtype=torch.bfloat16, device=self.device) if out_bf16 else None
        C32 = torch.empty((M, N), dtype=torch.float32, device=self.device) if out_f32 else None
        S = torch.empty((M, N), dtype=torch.bfloat16, device=self.device) if X2 is not None else None
        g.C, g.ldc, g.C32, g.ldc32 = _ptr(Cout), N, _ptr(C32), N
        g.bias, g.scale, g.shift = _ptr(bias), _ptr(scale), _ptr(shift)
        g.ubias, g.ldub = _ptr(ubias), (ubias.stride(0) if ubias is not None else 0)
        g.X2, g.ldx2 = _ptr(X2), (X2.stride(0) if X2 is not None else 0)
        g.S, g.lds = _ptr(S), N
        g.M, g.N, g.Cin, g.taps, g.dil, g.T = M, N, Cin, taps, dil, T
        g.flags = ((_lib.GEMM_RELU if relu else 0) | (_lib.GEMM_TANH if tanh else 0) | (_lib.GEMM_A_KBLOCKED if a_kblocked else 0)
                   | (_lib.GEMM_C_KBLOCKED if c_kblocked else 0))
        g.tap_pack = tap_pack
        part = None
        if stats_mode:
            part = torch.empty(self.lib.sdk_conv_gemm_stats_bytes(M, N, stats_mode), dtype=torch.uint8, device=self.device)
            g.stats_mode, g.stats_part = stats_mode, part.data_ptr()
        check(self.lib.sdk_conv_gemm(self.ctx, C.byref(g), _stream()), "sdk_conv_gemm")
        if stats_mode:
            st = torch.empty((M // T, N * stats_mode), dtype=torch.float32, device=self.device)
            check(self.lib.sdk_colstats_finish(self.ctx, part.data_ptr(), M, N, T, stats_mode, st.data_ptr(), _stream()), "sdk_colstats_finish")
            return Cout, C32, S, st
        return Cout, C32, S

    @staticmethod
    def to_kblocked(x: torch.Tensor) -> torch.Tensor:
        """[M, C] -> the K-blocked layout [C / 64, M, 64] (element (m, c) at (c // 64, m, c % 64)); for tests and tools."""
        M, Cc = x.shape
        return x.reshape(M, Cc // 64, 64).permute(1, 0, 2).contiguous()

    @staticmethod
    def from_kblocked(x: torch.Tensor) -> torch.Tensor:
        return x.permute(1, 0, 2).reshape(x.shape[1], x.shape[0] * 64).contiguous()

    # ---- precise mode building blocks (csrc/hp.hip) ------------------------------------------------
    @staticmethod
    def to_planes(x: torch.Tensor) -> torch.Tensor:
        """fp32 [M, C] -> fp16 planes [M, 2C]: hi | lo * 2^11 (the format csrc/hp.hpp stores; same arithmetic, for tests and tools)."""
        x = x.float().clamp(-65504.0, 65504.0)
        hi = x.to(torch.float16)
        lo = ((x - hi.float()) * 2048.0).to(torch.float16)
        return torch.cat([hi, lo], dim=1).contiguous()

    @staticmethod
    def from_planes(p: torch.Tensor) -> torch.Tensor:
        c = p.shape[1] // 2
        return p[:, :c].float() + p[:, c:].float() * (1.0 / 2048.0)

    def conv_gemm_hp(self, A, Wslot, N, Cin, taps=1, dil=1, T=None, bias=None, scale=None, shift=None, ubias=None,
                     relu=False, tanh=False, out_planes=True, out_f32=False, X2=None):
        """A: fp16 planes [M, 2*Cin']; Wslot: uint16/fp16 device tensor holding weights_pack.hp_weight_planes(W [N, taps*Cin]).
        Returns (C planes [M, 2N] or None, C32 fp32 or None, S planes or None)."""
        from ._lib import ConvGemmHpArgs
        _need(A, torch.float16, "A")
        M = A.shape[0]
        T = T or M
        g = ConvGemmHpArgs()
        g.A, g.lda, g.a_lo, g.W = A.data_ptr(), A.stride(0), A.shape[1] // 2, Wslot.data_ptr()
        Cout = torch.empty((M, 2 * N), dtype=torch.float16, device=self.device) if out_planes else None
        C32 = torch.empty((M, N), dtype=torch.float32, device=self.device) if out_f32 else None
        S = torch.empty((M, 2 * N), dtype=torch.float16, device=self.device) if X2 is not None else None
        g.C, g.ldc, g.c_lo, g.C32, g.ldc32 = _ptr(Cout), 2 * N, N, _ptr(C32), N
        g.bias, g.scale, g.shift = _ptr(bias), _ptr(scale), _ptr(shift)
        g.ubias, g.ldub = _ptr(ubias), (ubias.stride(0) if ubias is not None else 0)
        if X2 is not None:
            _need(X2, torch.float16, "X2")
            g.X2, g.ldx2, g.x2_lo = X2.data_ptr(), X2.stride(0), X2.shape[1] // 2
            g.S, g.lds, g.s_lo = S.data_ptr(), 2 * N, N
        g.M, g.N, g.Cin, g.taps, g.dil, g.T = M, N, Cin, taps, dil, T
        g.flags = (_lib.GEMM_RELU if relu else 0) | (_lib.GEMM_TANH if tanh else 0)
        check(self.lib.sdk_conv_gemm_hp(self.ctx, C.byref(g), _stream()), "sdk_conv_gemm_hp")
        return Cout, C32, S

    # the precise mode's sweeps, one kernel each (sdk_*_hp in csrc/hp.hip).  A plane operand is an fp16 tensor or view [B*T, >= lo + C] taken
    # as it is: row stride from the tensor, the lo plane `lo` columns to the right of the hi plane; the library checks the rest.
    def seg_mean_hp(self, z, z_lo, B, T, C_, out=None):
        """per-segment channel means of z planes -> [B, C] fp32 (out: a contiguous [B, C] fp32 tensor or view to write into)"""
        _need(z, torch.float16, "z")
        out = torch.empty((B, C_), dtype=torch.float32, device=self.device) if out is None else out
        check(self.lib.sdk_seg_mean_hp(self.ctx, z.data_ptr(), z.stride(0), z_lo, B, T, C_, out.data_ptr(), _stream()), "sdk_seg_mean_hp")
        return out

    def se_apply_hp(self, z, z_lo, x, x_lo, gate, out, o_lo, B, T, C_):
        """out planes = gate [B, C] fp32 * z + x, written into the caller's view `out` (hi plane at its column 0, lo plane o_lo to the right)"""
        _need(z, torch.float16, "z"); _need(x, torch.float16, "x"); _need(out, torch.float16, "out"); _need(gate, torch.float32, "gate")
        check(self.lib.sdk_se_apply_hp(self.ctx, z.data_ptr(), z.stride(0), z_lo, x.data_ptr(), x.stride(0), x_lo, gate.data_ptr(),
                                       out.data_ptr(), out.stride(0), o_lo, B, T, C_, _stream()), "sdk_se_apply_hp")
        return out

    def asp_stats_hp(self, h, h_lo, B, T, C_, out=None):
        """mean | std over frames of h planes -> [B, 2C] fp32"""
        _need(h, torch.float16, "h")
        out = torch.empty((B, 2 * C_), dtype=torch.float32, device=self.device) if out is None else out
        check(self.lib.sdk_asp_stats_hp(self.ctx, h.data_ptr(), h.stride(0), h_lo, B, T, C_, out.data_ptr(), _stream()), "sdk_asp_stats_hp")
        return out

    def asp_pool_hp(self, logits, h, h_lo, B, T, C_, out=None):
        """softmax over frames of fp32 logits [B*T, >= C] -> weighted mean | std of h planes -> [B, 2C] fp32"""
        _need(h, torch.float16, "h"); _need(logits, torch.float32, "logits")
        out = torch.empty((B, 2 * C_), dtype=torch.float32, device=self.device) if out is None else out
        check(self.lib.sdk_asp_pool_hp(self.ctx, logits.data_ptr(), logits.stride(0), h.data_ptr(), h.stride(0), h_lo, B, T, C_,
                                       out.data_ptr(), _stream()), "sdk_asp_pool_hp")
        return out

    def se_gate_residual(self, z, x, w1t, b1, w2t, b2, B, T, split: bool = True):
        C_ = z.shape[1]
        out = torch.empty_like(z)
        ws = self._scratch_bytes("se", self.lib.sdk_se_workspace_bytes(B, C_, w1t.shape[1])) if split else None
        fmt = _elem_fmt(z, "se_gate_residual")
        if x.dtype != z.dtype:
            raise ValueError(f"se_gate_residual: z is {z.dtype} but x is {x.dtype}")
        check(self.lib.sdk_se_gate_residual_fmt(self.ctx, z.data_ptr(), z.stride(0), x.data_ptr(), x.stride(0), w1t.data_ptr(),
                                                b1.data_ptr(), w2t.data_ptr(), b2.data_ptr(), out.data_ptr(), out.stride(0),
                                                B, T, C_, w1t.shape[1], None, _ptr(ws), ws.numel() if split else 0, fmt, _stream()),
              "sdk_se_gate_residual_fmt")
        return out

    def asp_stats(self, h, B, T):
        Cm = h.shape[1]
        out = torch.empty((B, 2 * Cm), dtype=torch.float32, device=self.device)
        check(self.lib.sdk_asp_stats_fmt(self.ctx, h.data_ptr(), h.stride(0), B, T, Cm, out.data_ptr(), _elem_fmt(h, "asp_stats"), _stream()),
              "sdk_asp_stats_fmt")
        return out

    def rows_fc(self, x, wt, bias=None, in_scale=None, in_shift=None, act=0):
        B, Cin = x.shape
        Nout = wt.shape[1]
        out = torch.empty((B, Nout), dtype=torch.float32, device=self.device)
        check(self.lib.sdk_rows_fc(self.ctx, x.data_ptr(), x.stride(0), _ptr(in_scale), _ptr(in_shift), wt.data_ptr(), _ptr(bias),
                                   out.data_ptr(), Nout, B, Cin, Nout, act, _stream()), "sdk_rows_fc")
        return out

    def asp_pool(self, logits, h, B, T):
        Cm = h.shape[1]
        out = torch.empty((B, 2 * Cm), dtype=torch.float32, device=self.device)
        check(self.lib.sdk_asp_pool_fmt(self.ctx, logits.data_ptr(), logits.stride(0), h.data_ptr(), h.stride(0), B, T, Cm,
                                        out.data_ptr(), _elem_fmt(h, "asp_pool"), _stream()), "sdk_asp_pool_fmt")
        return out


    # ------------------------------------------------------------------ k6 (spectral clustering pieces)
    def affinity_matvec(self, Eb, X, row0: int = 0, rows: Optional[int] = None, xscale=None, out=None):
        """Y[row0:row0+rows] = max(E E^T, 0)[row0:row0+rows, :] @ (xscale[:, None] * X);  X [N, kv] fp32."""
        _need(Eb, torch.bfloat16, "Eb"); _need(X, torch.float32, "X")
        N, d = Eb.shape
        kv = X.shape[1]
        rows = N - row0 if rows is None else rows
        Y = out if out is not None else torch.zeros((N, kv), dtype=torch.float32, device=self.device)
        ws = self._scratch_bytes("matvec", self.lib.sdk_affinity_matvec_workspace_bytes(N))
        check(self.lib.sdk_affinity_matvec(self.ctx, Eb.data_ptr(), N, d, row0, rows, X.contiguous().data_ptr(), _ptr(xscale), kv,
                                           Y.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "sdk_affinity_matvec")
        return Y

    def laplacian_topk(self, Eb_all, V0, n_iter: int, row0: int = 0, rows: Optional[int] = None, comm: Optional[int] = None, world: int = 1,
                       flag: Optional[torch.Tensor] = None):
        """The C-ABI spectral driver for non-Python hosts (sdk_laplacian_topk): top-k Ritz pairs of D^-1/2 A D^-1/2 by subspace iteration,
        never leaving the stream.  V0 [rows, k] fp32 start block (not modified) -> (U [rows, k], eigenvalues [k] device, descending).
        comm: an ncclComm_t as an integer (or None on one GPU)."""
        what = "laplacian_topk"
        # the C entry reads Eb_all as [N, 192] and V as [rows, k] through bare pointers: everything it cannot see is refused here, before
        # the scratch allocation and any launch
        _thin(Eb_all, "Eb_all", what, dtype=torch.bfloat16, contiguous=False)
        if Eb_all.dim() != 2 or Eb_all.shape[0] < 1 or Eb_all.shape[1] != 192:
            raise ValueError(f"{what}: Eb_all must be [N, 192] with N >= 1 (the width the mat-vec kernel is built for), got {list(Eb_all.shape)}")
        _thin(Eb_all, "Eb_all", what, dtype=torch.bfloat16)
        N = int(Eb_all.shape[0])
        if not (isinstance(row0, (int, np.integer)) and row0 >= 0):
            raise ValueError(f"{what}: row0 = {row0!r} must be an integer >= 0")
        rows = N - row0 if rows is None else rows
        if not (isinstance(rows, (int, np.integer)) and rows >= 1):
            raise ValueError(f"{what}: rows = {rows!r} must be an integer >= 1 (row0 = {row0}, N = {N})")
        if row0 + rows > N:
            raise ValueError(f"{what}: row0 + rows = {row0 + rows} exceeds the N = {N} rows of Eb_all")
        _thin(V0, "V0", what, contiguous=False)
        if V0.dim() != 2 or not 1 <= V0.shape[1] <= THIN_MAX:
            raise ValueError(f"{what}: V0 must be [rows, k] with k in 1..{THIN_MAX}, got {list(V0.shape)}")
        if V0.shape[0] != rows:
            raise ValueError(f"{what}: V0 must have rows = {rows} rows (one per owned row of Eb_all), got {list(V0.shape)}")
        if not (isinstance(n_iter, (int, np.integer)) and n_iter >= 0):
            raise ValueError(f"{what}: n_iter = {n_iter!r} must be an integer >= 0")
        if flag is not None:
            _thin(flag, "flag", what, dtype=torch.int32)
            if flag.numel() != 1:
                raise ValueError(f"{what}: flag must hold one int32, got shape {list(flag.shape)}")
        k = int(V0.shape[1])
        V = V0.contiguous().clone()
        lam = torch.empty((k,), dtype=torch.float32, device=self.device)
        ws = self._scratch_bytes("laplacian", self.lib.sdk_laplacian_topk_workspace_bytes(N, k))
        check(self.lib.sdk_laplacian_topk(self.ctx, Eb_all.data_ptr(), N, row0, rows, k, n_iter, V.data_ptr(), lam.data_ptr(), _ptr(flag), ws.data_ptr(),
                                          ws.numel(), comm, world, _stream()), "sdk_laplacian_topk")
        return V, lam

    def rows_gram(self, X, Y):
        """G [k, k] = X^T Y over the n rows of two contiguous fp32 [n, k] blocks (k <= 32)."""
        n, k = _thin_rows(X, "X", "rows_gram")
        _thin(Y, "Y", "rows_gram", shape=(n, k))
        G = torch.empty((k, k), dtype=torch.float32, device=self.device)
        ws = self._scratch_bytes("gram", self.lib.sdk_rows_gram_workspace_bytes(n, k))
        check(self.lib.sdk_rows_gram(self.ctx, X.data_ptr(), Y.data_ptr(), n, k, G.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "sdk_rows_gram")
        return G

    def rows_apply(self, X, R, scale=None):
        """Y[i, :] = scale[i] * (X[i, :] @ R): X contiguous fp32 [n, k], R fp32 [k, k], scale fp32 [n] or None."""
        n, k = _thin_rows(X, "X", "rows_apply")
        _thin(R, "R", "rows_apply", shape=(k, k), contiguous=False)
        if scale is not None:
            _thin(scale, "scale", "rows_apply", shape=(n,))
        Y = torch.empty_like(X)
        check(self.lib.sdk_rows_apply(self.ctx, X.data_ptr(), R.contiguous().data_ptr(), _ptr(scale), n, k, Y.data_ptr(), _stream()), "sdk_rows_apply")
        return Y

    def chol_inverse(self, G, flag: Optional[torch.Tensor] = None):
        """Rinv [k,k] with (G+G^T)/2 = L L^T, Rinv = (L^T)^-1 (float64 inside, stays on the stream).  `flag` (device int32 [1], zeroed
        by the caller) is set to 1 when G is not positive definite (rank-deficient or NaN input); it is sticky, so one flag can watch a
        whole iteration and be read at the caller's next host synchronisation."""
        k = G.shape[0]
        if flag is not None:
            _need(flag, torch.int32, "flag")
        Rinv = torch.empty((k, k), dtype=torch.float32, device=self.device)
        check(self.lib.sdk_chol_inverse(self.ctx, G.contiguous().data_ptr(), k, Rinv.data_ptr(), _ptr(flag), _stream()), "sdk_chol_inverse")
        return Rinv

    def sym_eigh(self, G):
        """(Q [k, k], lam [k]) fp32 on the device: every eigenpair of (G + G^T) / 2 for a contiguous fp32 G [k, k], 1 <= k <= 32 - the Ritz
        step of laplacian_topk alone (sdk_sym_eigh: cyclic Jacobi in float64, stays on the stream).  lam descending, equal eigenvalues in
        ascending order of their diagonal position; column c of Q belongs to lam[c], with its largest-magnitude component positive."""
        _thin(G, "G", "sym_eigh", contiguous=False)
        if G.dim() != 2 or G.shape[0] != G.shape[1]:
            raise ValueError(f"sym_eigh: G must be square [k, k], got {list(G.shape)}")
        k = int(G.shape[0])
        if not 1 <= k <= THIN_MAX:
            raise ValueError(f"sym_eigh: k = {k} (the order of G) must be in 1..{THIN_MAX}")
        _thin(G, "G", "sym_eigh")
        Q = torch.empty((k, k), dtype=torch.float32, device=self.device)
        lam = torch.empty((k,), dtype=torch.float32, device=self.device)
        check(self.lib.sdk_sym_eigh(self.ctx, G.data_ptr(), k, Q.data_ptr(), lam.data_ptr(), _stream()), "sdk_sym_eigh")
        return Q, lam

    def rows_unit(self, X):
        """The rows of a contiguous fp32 [n, k] block scaled to unit length (a row shorter than 1e-12 is divided by 1e-12: a zero row stays zero)."""
        n, k = _thin_rows(X, "X", "rows_unit")
        Y = torch.empty_like(X)
        check(self.lib.sdk_rows_unit(self.ctx, X.data_ptr(), n, k, Y.data_ptr(), _stream()), "sdk_rows_unit")
        return Y

    def kmeans_mindist(self, R, centre, d2, first: bool):
        """d2[i] = |R[i] - centre|^2 (first) or min(d2[i], that), in place: R contiguous fp32 [n, k], centre fp32 [k], d2 contiguous fp32 [n]."""
        n, k = _thin_rows(R, "R", "kmeans_mindist")
        _thin(centre, "centre", "kmeans_mindist", shape=(k,), contiguous=False)
        _thin(d2, "d2", "kmeans_mindist", shape=(n,))
        check(self.lib.sdk_kmeans_mindist(self.ctx, R.data_ptr(), n, k, centre.contiguous().data_ptr(), d2.data_ptr(), int(first), _stream()), "sdk_kmeans_mindist")
        return d2

    def kmeans_assign(self, R, centres, want_sums: bool = True):
        """One k-means step on the contiguous fp32 rows R [n, k] against centres fp32 [kc, k] (k, kc <= 32) ->
        (label int32 [n], dist2 fp32 [n], part_sum fp32 [ceil(n / 256), kc, k], part_cnt int32 [ceil(n / 256), kc]); the last two are None
        without want_sums.  label is the nearest centre, ties to the lowest index; part_sum / part_cnt are the sums and counts of each
        block of 256 rows per label, added in ascending row order (reproducible).
        A row that holds a NaN (or whose distance to every centre is NaN, as with NaN centres) compares below nothing: it gets label -1 and
        dist2 +inf and enters no sum and no count; the other rows of its block are not affected.  cluster.canonical_labels refuses a
        negative label."""
        n, k = _thin_rows(R, "R", "kmeans_assign")
        _thin(centres, "centres", "kmeans_assign", contiguous=False)
        if centres.dim() != 2 or centres.shape[1] != k:
            raise ValueError(f"kmeans_assign: centres must be [kc, k] with k = {k} (the width of R), got {list(centres.shape)}")
        kc = int(centres.shape[0])
        if not 1 <= kc <= THIN_MAX:
            raise ValueError(f"kmeans_assign: kc = {kc} (the rows of centres) must be in 1..{THIN_MAX}")
        lab = torch.empty((n,), dtype=torch.int32, device=self.device)
        d2 = torch.empty((n,), dtype=torch.float32, device=self.device)
        nb = (n + 255) // 256
        ps = torch.empty((nb, kc, k), dtype=torch.float32, device=self.device) if want_sums else None
        pc = torch.empty((nb, kc), dtype=torch.int32, device=self.device) if want_sums else None
        check(self.lib.sdk_kmeans_assign(self.ctx, R.data_ptr(), n, k, centres.contiguous().data_ptr(), kc, lab.data_ptr(), d2.data_ptr(),
                                         _ptr(ps), _ptr(pc), _stream()), "sdk_kmeans_assign")
        return lab, d2, ps, pc

    # ------------------------------------------------------------------ k6 (threshold path: centroid-linkage agglomerative clustering)
    def centroid_linkage(self, E: torch.Tensor, offsets=None) -> torch.Tensor:
        """E [N, d] fp32 unit rows (device) -> Z float64 [N - G, 4] (device): scipy's centroid linkage of every problem, in its layout and
        numbering.  offsets (host, G + 1 strictly increasing row bounds; None = one problem of all N rows): problem g's n_g - 1 rows start at
        row offsets[g] - g.  Raises ValueError naming the problem when one holds a non-finite row (its rows of Z are then not written; the
        exception carries .linkage, with the other problems' rows valid, and .status [G])."""
        _need(E, torch.float32, "E")
        if E.dim() != 2 or E.stride(1) != 1:
            E = E.contiguous()
        N, d = E.shape
        off = np.asarray([0, N] if offsets is None else offsets, dtype=np.int64)
        if off.ndim != 1 or off.size < 2 or off[0] != 0 or off[-1] != N:
            raise ValueError(f"centroid_linkage: offsets must run from 0 to N = {N}, got {off.tolist()[:8]}")
        off32 = np.ascontiguousarray(off.astype(np.int32))
        G = off32.size - 1
        op = off32.ctypes.data_as(C.POINTER(C.c_int32))
        nbytes = self.lib.sdk_centroid_linkage_workspace_bytes(op, G, d)
        if nbytes == 0:
            raise SdkError(f"sdk_centroid_linkage_workspace_bytes: {self.lib.sdk_last_error().decode()}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        Zbuf = torch.empty((max(N - G, 1), 4), dtype=torch.float64, device=self.device)   # never a null pointer (G single-row problems: no rows)
        status = torch.empty((G,), dtype=torch.int32, device=self.device)
        check(self.lib.sdk_centroid_linkage(self.ctx, E.data_ptr(), E.stride(0), d, op, G, Zbuf.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                            nbytes, _stream()), "sdk_centroid_linkage")
        Z = Zbuf[:N - G]
        st = status.cpu().numpy()
        bad = np.flatnonzero(st)
        if bad.size:
            g = int(bad[0])
            err = ValueError(f"centroid_linkage: problem {g} (rows {int(off[g])} .. {int(off[g + 1])}) has a non-finite row or distance "
                             f"(status {int(st[g])}); problems with one: {bad.tolist()[:16]}")
            err.linkage, err.status = Z, st             # the other problems' rows of Z are valid
            raise err
        return Z

    def linked_linkage(self, E: torch.Tensor, group: torch.Tensor, offsets=None, stop=None):
        """E [N, d] fp32 unit rows, group [N] int32 (device) -> (Z float64 [N - G, 4], merges int32 [G]) on the device: the linked centroid
        linkage of every problem (sdk_linked_linkage; the rule heads csrc/ahc.hip).  Rows of one problem that share a group >= 0 never
        share a cluster (a negative group is a free row); each step merges the allowed pair of least centroid distance and the problem ends
        when none is left or that distance exceeds stop (None: +inf).  Problem g's rows of Z start at offsets[g] - g as in centroid_linkage;
        the rows from merges[g] on are zero.  Raises ValueError naming the problem when one holds a non-finite row, as centroid_linkage
        does (.linkage, .merges and .status on the exception)."""
        _need(E, torch.float32, "E")
        _need(group, torch.int32, "group")
        if E.dim() != 2 or E.stride(1) != 1:
            E = E.contiguous()
        N, d = E.shape
        if group.dim() != 1 or group.numel() != N:
            raise ValueError(f"linked_linkage: group must be [N] = [{N}], got {list(group.shape)}")
        group = group.contiguous()
        stop = float("inf") if stop is None else float(stop)
        if not stop >= 0.0:
            raise ValueError(f"linked_linkage: stop={stop} (a distance >= 0, or None / +inf for every allowed merge)")
        off = np.asarray([0, N] if offsets is None else offsets, dtype=np.int64)
        if off.ndim != 1 or off.size < 2 or off[0] != 0 or off[-1] != N:
            raise ValueError(f"linked_linkage: offsets must run from 0 to N = {N}, got {off.tolist()[:8]}")
        off32 = np.ascontiguousarray(off.astype(np.int32))
        G = off32.size - 1
        op = off32.ctypes.data_as(C.POINTER(C.c_int32))
        nbytes = self.lib.sdk_linked_linkage_workspace_bytes(op, G, d)
        if nbytes == 0:
            raise SdkError(f"sdk_linked_linkage_workspace_bytes: {self.lib.sdk_last_error().decode()}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        Zbuf = torch.empty((max(N - G, 1), 4), dtype=torch.float64, device=self.device)   # never a null pointer
        merges = torch.empty((G,), dtype=torch.int32, device=self.device)
        status = torch.empty((G,), dtype=torch.int32, device=self.device)
        check(self.lib.sdk_linked_linkage(self.ctx, E.data_ptr(), E.stride(0), d, group.data_ptr(), op, G, stop, Zbuf.data_ptr(), merges.data_ptr(),
                                          status.data_ptr(), ws.data_ptr(), nbytes, _stream()), "sdk_linked_linkage")
        Z = Zbuf[:N - G]
        st = status.cpu().numpy()
        bad = np.flatnonzero(st)
        if bad.size:
            g = int(bad[0])
            err = ValueError(f"linked_linkage: problem {g} (rows {int(off[g])} .. {int(off[g + 1])}) has a non-finite row or distance "
                             f"(status {int(st[g])}); problems with one: {bad.tolist()[:16]}")
            err.linkage, err.merges, err.status = Z, merges, st     # the other problems' rows of Z are valid
            raise err
        return Z, merges

    # ---- streaming diarization (stream.py; csrc/stream.hip): a bank's speaker tables and frame rings live in one device block
    def stream_state(self, n_streams: int, capacity: int, d: int) -> "StreamState":
        """The device state of a bank of n_streams live streams (capacity speakers each, embedding width d), reset, with the output rows
        that stream_step and stream_flush write."""
        nbytes = int(self.lib.sdk_stream_state_bytes(int(n_streams), int(capacity), int(d)))
        if nbytes == 0:
            raise ValueError(f"stream_state: n_streams={n_streams} (at least 1), capacity={capacity} (1 .. 64), d={d} (a multiple of 64, at most 512)")
        st = StreamState(self, int(n_streams), int(capacity), int(d), nbytes)
        self.stream_reset(st)
        return st

    def stream_reset(self, st: "StreamState", which: Optional[torch.Tensor] = None) -> None:
        """Empty the speaker table and the ring of the streams with which[r] != 0 (uint8 [R], device); None: of every stream."""
        if which is not None:
            which = _thin(which, "which", "stream_reset", (st.R,), torch.uint8)
        check(self.lib.sdk_stream_reset(self.ctx, st.buf.data_ptr(), st.nbytes, st.R, st.capacity, st.d, _ptr(which), _stream()), "sdk_stream_reset")

    def stream_step(self, st: "StreamState", E: torch.Tensor, info: torch.Tensor, cls: torch.Tensor, starts: torch.Tensor, active: torch.Tensor,
                    hop: int, latency: int, delta_new: float = 1.0, max_speakers: Optional[int] = None,
                    n_end: Optional[torch.Tensor] = None) -> "StreamState":
        """One bank step (sdk_stream_step): stream r's chunk is E [3 r .. 3 r + 2] (unit fp32 rows), info [r] (int32 [3, 4]), cls [r] (uint8 [F])
        and starts [r] (int64, samples); streams with active [r] == 0 (uint8) are left alone.  hop and latency in samples.  n_end (int64 [R], or None): n_end [r] > 0 says
        that the chunk is stream r's last and where the stream ends; no frame beyond that end is emitted.  The results stand
        in st.labels, st.score, st.K, st.emit_lo, st.emit_n, st.count and st.speakers (device), rows of inactive streams untouched."""
        R, d = st.R, st.d
        _thin(E, "E", "stream_step", (3 * R, d))
        _thin(info, "info", "stream_step", (R, 3, 4), torch.int32)
        _thin(cls, "cls", "stream_step", None, torch.uint8)
        if cls.dim() != 2 or cls.shape[0] != R:
            raise ValueError(f"stream_step: cls must be [{R}, F], got {list(cls.shape)}")
        _thin(starts, "starts", "stream_step", (R,), torch.int64)
        _thin(active, "active", "stream_step", (R,), torch.uint8)
        if n_end is not None:
            _thin(n_end, "n_end", "stream_step", (R,), torch.int64)
        cap = 2 if max_speakers is None else int(max_speakers)
        check(self.lib.sdk_stream_step(self.ctx, E.data_ptr(), info.data_ptr(), cls.data_ptr(), starts.data_ptr(), active.data_ptr(), _ptr(n_end), R, int(cls.shape[1]),
                                       d, st.capacity, int(hop), int(latency), float(delta_new), cap, st.buf.data_ptr(), st.nbytes,
                                       st.labels.data_ptr(), st.score.data_ptr(), st.K.data_ptr(), st.emit_lo.data_ptr(), st.emit_n.data_ptr(),
                                       st.count.data_ptr(), st.speakers.data_ptr(), _stream()), "sdk_stream_step")
        return st

    def stream_flush(self, st: "StreamState", n_samples: torch.Tensor, active: torch.Tensor, max_speakers: Optional[int] = None) -> "StreamState":
        """The end of the streams with active [r] != 0 at n_samples [r] (int64, device): every frame not yet emitted stands in st.emit_lo,
        st.emit_n, st.count and st.speakers (sdk_stream_flush)."""
        _thin(n_samples, "n_samples", "stream_flush", (st.R,), torch.int64)
        _thin(active, "active", "stream_flush", (st.R,), torch.uint8)
        cap = 2 if max_speakers is None else int(max_speakers)
        check(self.lib.sdk_stream_flush(self.ctx, n_samples.data_ptr(), active.data_ptr(), st.R, st.capacity, st.d, cap, st.buf.data_ptr(), st.nbytes,
                                        st.emit_lo.data_ptr(), st.emit_n.data_ptr(), st.count.data_ptr(), st.speakers.data_ptr(), _stream()),
              "sdk_stream_flush")
        return st

    def stream_centroids(self, st: "StreamState", first: int = 0, count: Optional[int] = None, sums: bool = False):
        """Of the streams first .. first + count - 1 (count None: to the last) -> (cent [count, capacity, d] fp32 unit rows, zero from K [r]
        on; counts [count, capacity] int32; K [count] int32) on the device; sums=True: and the float64 sums [count, capacity, d]."""
        count = st.R - int(first) if count is None else int(count)
        if not (0 <= int(first) and 1 <= count <= st.R - int(first)):
            raise ValueError(f"stream_centroids: streams first={first}, count={count} of {st.R}")
        cent = torch.empty((count, st.capacity, st.d), dtype=torch.float32, device=self.device)
        counts = torch.empty((count, st.capacity), dtype=torch.int32, device=self.device)
        K = torch.empty((count,), dtype=torch.int32, device=self.device)
        S = torch.empty((count, st.capacity, st.d), dtype=torch.float64, device=self.device) if sums else None
        check(self.lib.sdk_stream_centroids(self.ctx, st.buf.data_ptr(), st.nbytes, st.R, st.capacity, st.d, int(first), count, cent.data_ptr(),
                                            counts.data_ptr(), K.data_ptr(), _ptr(S), _stream()), "sdk_stream_centroids")
        return (cent, counts, K, S) if sums else (cent, counts, K)

    # ---- VBx clustering (cluster.vbx_cluster, plda.py; csrc/vbx.hip): nothing here synchronises with the host except the range check of rows
    @staticmethod
    def _vbx_rows(name: str, E: torch.Tensor, rows: torch.Tensor, check_rows: bool) -> int:
        if E.dim() != 2 or E.dtype != torch.float32 or not E.is_contiguous() or not E.is_cuda:
            raise ValueError(f"{name}: E must be a contiguous fp32 [rows, d] device tensor, got {tuple(E.shape)} {E.dtype}")
        if E.shape[1] < 64 or E.shape[1] % 64 or E.shape[1] > 512:
            raise ValueError(f"{name}: d={E.shape[1]} not supported (a multiple of 64, at most 512)")
        if rows.dim() != 1 or rows.dtype != torch.int32 or not rows.is_contiguous() or not rows.is_cuda:
            raise ValueError(f"{name}: rows must be a contiguous int32 [n] device tensor, got {tuple(rows.shape)} {rows.dtype}")
        n = int(rows.numel())
        if n < 1 or n > 65536:
            raise ValueError(f"{name}: n={n} rows (1 .. 65536)")
        if check_rows and not (0 <= int(rows.min()) and int(rows.max()) < E.shape[0]):      # the kernels read E at these rows
            raise ValueError(f"{name}: rows must lie in [0, {E.shape[0]}), got {int(rows.min())} .. {int(rows.max())}")
        return n

    def plda_transform(self, E: torch.Tensor, rows: torch.Tensor, plda, check_rows: bool = True) -> torch.Tensor:
        """E [R, d_in] fp32 unit rows, rows [n] int32 (device), plda a plda.Plda -> X [n, D] float64 (device): sdk_plda_transform.
        check_rows=False: the caller has checked that rows lie in [0, R) (the check reads them back)."""
        n = self._vbx_rows("plda_transform", E, rows, check_rows)
        if int(E.shape[1]) != plda.d_in:
            raise ValueError(f"plda_transform: E has d={E.shape[1]}, the PLDA model takes d_in={plda.d_in}")
        D = int(plda.lda_dim)
        if D not in (64, 128) or D > plda.D0:
            raise ValueError(f"plda_transform: D={D} not supported (64 or 128, at most D0={plda.D0})")
        m = plda.device_arrays(E.device)
        X = torch.empty((n, D), dtype=torch.float64, device=E.device)
        check(self.lib.sdk_plda_transform(self.ctx, E.data_ptr(), plda.d_in, rows.data_ptr(), n, m["mean1"].data_ptr(), m["lda"].data_ptr(),
                                          m["mean2"].data_ptr(), m["mu"].data_ptr(), m["Tt"].data_ptr(), plda.D0, D, X.data_ptr(), _stream()),
              "sdk_plda_transform")
        return X

    def vbx(self, X: torch.Tensor, Phi: torch.Tensor, labels: torch.Tensor, S: int, Fa: float = 0.07, Fb: float = 0.8, max_iters: int = 20,
            epsilon: float = 1e-4, init_smoothing: float = 7.0):
        """X [n, D] float64, Phi [D] float64, labels [n] int32 in [0, S) (all on the device) -> (gamma [n, S], pi [S], elbo [max_iters],
        n_iter [1] int32, status [1] int32), all on the device and not read back: sdk_vbx.  The caller reads n_iter and status once."""
        return self._vbx("vbx", None, X, Phi, labels, S, Fa, Fb, max_iters, epsilon, init_smoothing)

    def vbx_hmm(self, X: torch.Tensor, Phi: torch.Tensor, labels: torch.Tensor, S: int, loop_prob: float, Fa: float = 0.07, Fb: float = 0.8,
                max_iters: int = 20, epsilon: float = 1e-4, init_smoothing: float = 7.0):
        """vbx with the HMM: the rows of X are a sequence in time order and loop_prob in [0, 1) is the probability that a row keeps the speaker
        of the row before it (sdk_vbx_hmm).  The same five device tensors."""
        loop_prob = float(loop_prob)
        if not 0.0 <= loop_prob < 1.0:                                    # a NaN fails both
            raise ValueError(f"vbx_hmm: loop_prob={loop_prob} (at least 0, below 1)")
        return self._vbx("vbx_hmm", loop_prob, X, Phi, labels, S, Fa, Fb, max_iters, epsilon, init_smoothing)

    def _vbx(self, who, loop_prob, X, Phi, labels, S, Fa, Fb, max_iters, epsilon, init_smoothing):
        if X.dim() != 2 or X.dtype != torch.float64 or not X.is_contiguous() or not X.is_cuda:
            raise ValueError(f"{who}: X must be a contiguous float64 [n, D] device tensor, got {tuple(X.shape)} {X.dtype}")
        n, D = int(X.shape[0]), int(X.shape[1])
        if D not in (64, 128):
            raise ValueError(f"{who}: D={D} not supported (64 or 128)")
        if n < 1 or n > 65536:
            raise ValueError(f"{who}: n={n} rows (1 .. 65536)")
        if Phi.dtype != torch.float64 or tuple(Phi.shape) != (D,) or not Phi.is_contiguous() or not Phi.is_cuda:
            raise ValueError(f"{who}: Phi must be a contiguous float64 [{D}] device tensor, got {tuple(Phi.shape)} {Phi.dtype}")
        if labels.dtype != torch.int32 or tuple(labels.shape) != (n,) or not labels.is_contiguous() or not labels.is_cuda:
            raise ValueError(f"{who}: labels must be a contiguous int32 [{n}] device tensor, got {tuple(labels.shape)} {labels.dtype}")
        S, max_iters = int(S), int(max_iters)
        if S < 1 or S > 65536:
            raise ValueError(f"{who}: S={S} (1 .. 65536)")
        if max_iters < 1 or max_iters > 1000:
            raise ValueError(f"{who}: max_iters={max_iters} (1 .. 1000)")
        Fa, Fb, epsilon, init_smoothing = float(Fa), float(Fb), float(epsilon), float(init_smoothing)
        if not (0 < Fa < np.inf and 0 < Fb < np.inf) or epsilon != epsilon or not (0 <= init_smoothing < np.inf):
            raise ValueError(f"{who}: Fa={Fa} Fb={Fb} (positive, finite), epsilon={epsilon} (not NaN), init_smoothing={init_smoothing} (finite, >= 0)")
        sizer = "sdk_vbx_workspace_bytes" if loop_prob is None else "sdk_vbx_hmm_workspace_bytes"
        nbytes = getattr(self.lib, sizer)(n, D, S)
        if nbytes == 0:
            raise SdkError(f"{sizer}: {self.lib.sdk_last_error().decode()}")
        dev = X.device
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        gamma = torch.empty((n, S), dtype=torch.float64, device=dev)
        pi = torch.empty((S,), dtype=torch.float64, device=dev)
        elbo = torch.empty((max_iters,), dtype=torch.float64, device=dev)
        n_iter = torch.empty((1,), dtype=torch.int32, device=dev)
        status = torch.empty((1,), dtype=torch.int32, device=dev)
        head = (self.ctx, X.data_ptr(), Phi.data_ptr(), labels.data_ptr(), n, D, S, Fa, Fb, max_iters, epsilon, init_smoothing)
        tail = (gamma.data_ptr(), pi.data_ptr(), elbo.data_ptr(), n_iter.data_ptr(), status.data_ptr(), ws.data_ptr(), nbytes, _stream())
        if loop_prob is None:
            check(self.lib.sdk_vbx(*head, *tail), "sdk_vbx")
        else:
            check(self.lib.sdk_vbx_hmm(*head, loop_prob, *tail), "sdk_vbx_hmm")
        return gamma, pi, elbo, n_iter, status

    def vbx_centroids(self, gamma: torch.Tensor, pi: torch.Tensor, E: torch.Tensor, rows: torch.Tensor, check_rows: bool = True):
        """gamma [n, S], pi [S] float64, E [R, d] fp32 unit rows, rows [n] int32 (all on the device) -> (K [1] int32, keep [S] int32,
        labels [n] int32, cent [S, d] fp32, cent64 [S, d] float64) on the device: sdk_vbx_centroids.  Rows K.. of the centroids are zeros."""
        n = self._vbx_rows("vbx_centroids", E, rows, check_rows)
        if gamma.dim() != 2 or gamma.dtype != torch.float64 or gamma.shape[0] != n or not gamma.is_contiguous() or not gamma.is_cuda or gamma.shape[1] < 1:
            raise ValueError(f"vbx_centroids: gamma must be a contiguous float64 [{n}, S] device tensor, got {tuple(gamma.shape)} {gamma.dtype}")
        S, d = int(gamma.shape[1]), int(E.shape[1])
        if pi.dtype != torch.float64 or tuple(pi.shape) != (S,) or not pi.is_contiguous() or not pi.is_cuda:
            raise ValueError(f"vbx_centroids: pi must be a contiguous float64 [{S}] device tensor, got {tuple(pi.shape)} {pi.dtype}")
        dev = E.device
        K = torch.empty((1,), dtype=torch.int32, device=dev)
        keep = torch.empty((S,), dtype=torch.int32, device=dev)
        labels = torch.empty((n,), dtype=torch.int32, device=dev)
        cent = torch.zeros((S, d), dtype=torch.float32, device=dev)
        cent64 = torch.zeros((S, d), dtype=torch.float64, device=dev)
        check(self.lib.sdk_vbx_centroids(self.ctx, gamma.data_ptr(), pi.data_ptr(), E.data_ptr(), rows.data_ptr(), n, S, d, K.data_ptr(), keep.data_ptr(),
                                         labels.data_ptr(), cent.data_ptr(), cent64.data_ptr(), _stream()), "sdk_vbx_centroids")
        return K, keep, labels, cent, cent64

    # ---- training the PLDA from labelled rows (plda.fit; csrc/plda_fit.hip)
    def plda_fit_stats(self, rows: torch.Tensor, labels: Optional[torch.Tensor] = None, K: int = 0, mean1: Optional[torch.Tensor] = None,
                       scatter: bool = True, check_labels: bool = True) -> dict:
        """rows [N, d] on the device: fp32 (d a multiple of 64, at most 512; with mean1 [d] float64 every row enters as
        sqrt(d) unit(e - mean1)) or float64 as they lie (d 1 .. 512); labels [N] int32 in [0, K) or None (K = 0: the total and the scatter
        only) -> dict(counts [K] int64, sums [K, d], total [d], scatter [d, d] or None, status [1] int32), float64 on the device:
        sdk_plda_fit_stats.  The labels' range is checked here, before any launch (one read-back; check_labels=False: the caller has), and the
        row indices are sorted by label with torch's stable sort."""
        if rows.dim() != 2 or rows.dtype not in (torch.float32, torch.float64) or not rows.is_contiguous() or not rows.is_cuda:
            raise ValueError(f"plda_fit_stats: rows must be a contiguous fp32 or float64 [N, d] device tensor, got {tuple(rows.shape)} {rows.dtype}")
        N, d, K = int(rows.shape[0]), int(rows.shape[1]), int(K)
        f32 = rows.dtype == torch.float32
        if N < 1 or N > 1 << 24:
            raise ValueError(f"plda_fit_stats: N={N} rows (1 .. 2^24)")
        if (d < 64 or d % 64 or d > 512) if f32 else (d < 1 or d > 512):
            raise ValueError(f"plda_fit_stats: d={d} not supported (fp32 rows: a multiple of 64 in 64 .. 512; float64 rows: 1 .. 512)")
        if mean1 is not None and (not f32 or mean1.dtype != torch.float64 or tuple(mean1.shape) != (d,) or not mean1.is_contiguous() or not mean1.is_cuda):
            raise ValueError(f"plda_fit_stats: mean1 goes with fp32 rows and must be a contiguous float64 [{d}] device tensor")
        if K < 0 or K > 1 << 24 or (labels is None) != (K == 0):
            raise ValueError(f"plda_fit_stats: K={K} (1 .. 2^24 with labels, 0 without)")
        dev = rows.device
        order = counts = sums = None
        if labels is not None:
            if labels.dtype != torch.int32 or tuple(labels.shape) != (N,) or not labels.is_contiguous() or not labels.is_cuda:
                raise ValueError(f"plda_fit_stats: labels must be a contiguous int32 [{N}] device tensor, got {tuple(labels.shape)} {labels.dtype}")
            if check_labels:
                lo, hi = int(labels.min()), int(labels.max())
                if lo < 0 or hi >= K:
                    raise ValueError(f"plda_fit_stats: labels must lie in [0, {K}), got {lo} .. {hi}")
            order = torch.sort(labels, stable=True).indices.to(torch.int32)
            counts = torch.empty((K,), dtype=torch.int64, device=dev)
            sums = torch.empty((K, d), dtype=torch.float64, device=dev)
        nbytes = int(self.lib.sdk_plda_fit_stats_workspace_bytes(N, d, K, int(bool(scatter))))
        if nbytes == 0:
            raise SdkError(f"sdk_plda_fit_stats_workspace_bytes: {self.lib.sdk_last_error().decode()}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        total = torch.empty((d,), dtype=torch.float64, device=dev)
        S = torch.empty((d, d), dtype=torch.float64, device=dev) if scatter else None
        status = torch.empty((1,), dtype=torch.int32, device=dev)
        check(self.lib.sdk_plda_fit_stats(self.ctx, rows.data_ptr() if f32 else None, None if f32 else rows.data_ptr(), _ptr(mean1), N, d, _ptr(labels),
                                          _ptr(order), K, _ptr(counts), _ptr(sums), total.data_ptr(), _ptr(S), status.data_ptr(), ws.data_ptr(), nbytes,
                                          _stream()), "sdk_plda_fit_stats")
        return dict(counts=counts, sums=sums, total=total, scatter=S, status=status)

    def plda_project(self, E: torch.Tensor, mean1: torch.Tensor, lda: torch.Tensor, mean2: torch.Tensor) -> torch.Tensor:
        """E [N, d_in] fp32 rows, mean1 [d_in], lda [d_in, D0], mean2 [D0] (float64, device) -> x2 [N, D0] float64:
        sqrt(D0) unit(lda^T sqrt(d_in) unit(e - mean1) - mean2), sdk_plda_transform's first two steps for every row (sdk_plda_project)."""
        if E.dim() != 2 or E.dtype != torch.float32 or not E.is_contiguous() or not E.is_cuda:
            raise ValueError(f"plda_project: E must be a contiguous fp32 [N, d] device tensor, got {tuple(E.shape)} {E.dtype}")
        N, d_in = int(E.shape[0]), int(E.shape[1])
        if N < 1 or N > 1 << 24:
            raise ValueError(f"plda_project: N={N} rows (1 .. 2^24)")
        if d_in < 64 or d_in % 64 or d_in > 512:
            raise ValueError(f"plda_project: d_in={d_in} not supported (a multiple of 64, at most 512)")
        if lda.dim() != 2 or lda.shape[0] != d_in or not 1 <= lda.shape[1] <= 512:
            raise ValueError(f"plda_project: lda must be [{d_in}, D0 <= 512], got {tuple(lda.shape)}")
        D0 = int(lda.shape[1])
        for name, t, shape in (("mean1", mean1, (d_in,)), ("lda", lda, (d_in, D0)), ("mean2", mean2, (D0,))):
            if t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda:
                raise ValueError(f"plda_project: {name} must be a contiguous float64 {list(shape)} device tensor, got {tuple(t.shape)} {t.dtype}")
        X2 = torch.empty((N, D0), dtype=torch.float64, device=E.device)
        check(self.lib.sdk_plda_project(self.ctx, E.data_ptr(), d_in, N, mean1.data_ptr(), lda.data_ptr(), mean2.data_ptr(), D0, X2.data_ptr(),
                                        _stream()), "sdk_plda_project")
        return X2

    # ---- PLDA log-likelihood-ratio scoring (plda_score.py; csrc/plda_score.hip): nothing here synchronises with the host
    @staticmethod
    def _plda_f64(who: str, name: str, t, shape) -> None:
        """A float64 argument of the PLDA scoring calls: a contiguous device tensor of exactly `shape` (None: any extent)."""
        want = "[" + ", ".join("*" if s is None else str(s) for s in shape) + "]"
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.dim() != len(shape) or not t.is_contiguous() or not t.is_cuda \
                or any(s is not None and int(t.shape[i]) != s for i, s in enumerate(shape)):
            raise ValueError(f"{who}: {name} must be a contiguous float64 {want} device tensor, got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__} {getattr(t, 'dtype', '')}")

    def plda_enroll(self, Xp: torch.Tensor, group: torch.Tensor, n_eff: torch.Tensor, Phi: torch.Tensor):
        """Xp [P, D] float64 transformed profile rows (plda_transform; D 64 or 128, P <= 2^22), group [P] int32 (the speaker index of every
        row, in any order), n_eff [S] float64 (1 <= S <= 2^20), Phi [D] float64, all on the device -> (G [S, 2 D], r [S], status [1] int32)
        on the device: the speaker table of plda_score.py (sdk_plda_enroll).  A label outside [0, S) belongs to no speaker and sets status
        bit 1; a speaker without a row or with an n_eff that is not a finite number above 0 gets r = NaN.  The caller reads status."""
        self._plda_f64("plda_enroll", "Xp", Xp, (None, None))
        P, D = int(Xp.shape[0]), int(Xp.shape[1])
        if D not in (64, 128):
            raise ValueError(f"plda_enroll: D={D} not supported (64 or 128)")
        if P > 1 << 22:
            raise ValueError(f"plda_enroll: P={P} rows (0 .. 2^22)")
        if not isinstance(group, torch.Tensor) or group.dtype != torch.int32 or tuple(group.shape) != (P,) or not group.is_contiguous() or not group.is_cuda:
            raise ValueError(f"plda_enroll: group must be a contiguous int32 [{P}] device tensor, got "
                             f"{tuple(group.shape) if isinstance(group, torch.Tensor) else type(group).__name__} {getattr(group, 'dtype', '')}")
        self._plda_f64("plda_enroll", "n_eff", n_eff, (None,))
        S = int(n_eff.shape[0])
        if S < 1 or S > 1 << 20:
            raise ValueError(f"plda_enroll: S={S} speakers (1 .. 2^20)")
        self._plda_f64("plda_enroll", "Phi", Phi, (D,))
        nbytes = int(self.lib.sdk_plda_enroll_workspace_bytes(P, S))
        if nbytes == 0:
            raise SdkError(f"sdk_plda_enroll_workspace_bytes: {self.lib.sdk_last_error().decode()}")
        dev = Xp.device
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        G = torch.empty((S, 2 * D), dtype=torch.float64, device=dev)
        r = torch.empty((S,), dtype=torch.float64, device=dev)
        status = torch.empty((1,), dtype=torch.int32, device=dev)
        check(self.lib.sdk_plda_enroll(self.ctx, Xp.data_ptr() if P else None, group.data_ptr() if P else None, P, D, n_eff.data_ptr(),
                                       Phi.data_ptr(), S, G.data_ptr(), r.data_ptr(), status.data_ptr(), ws.data_ptr(), nbytes, _stream()),
              "sdk_plda_enroll")
        return G, r, status

    def plda_score_topk(self, X: torch.Tensor, G: torch.Tensor, r: torch.Tensor, k: int = 1, scores: bool = False,
                        ws: Optional[torch.Tensor] = None):
        """X [N, D] float64 transformed windows (N <= 65 536), (G [S, 2 D], r [S]) a speaker table of plda_enroll -> (idx [N, k] int32,
        score [N, k] float64) and, with scores=True, the whole matrix [N, S]: per window the k <= 4 largest log-likelihood ratios
        r_s + sum_d x_d G[s, d] + x_d^2 G[s, D + d]; ties to the lower speaker, a NaN never taken, a slot without a candidate holds
        (-1, 0); with k > S the columns S .. k - 1 are not written (sdk_plda_score_topk).  ws: a uint8 device tensor to use as the workspace
        (default: one of sdk_plda_score_workspace_bytes(N, S, k) bytes is allocated)."""
        self._plda_f64("plda_score_topk", "X", X, (None, None))
        N, D = int(X.shape[0]), int(X.shape[1])
        if D not in (64, 128):
            raise ValueError(f"plda_score_topk: D={D} not supported (64 or 128)")
        if N > 65536:
            raise ValueError(f"plda_score_topk: N={N} windows (0 .. 65536)")
        self._plda_f64("plda_score_topk", "G", G, (None, 2 * D))
        S, k = int(G.shape[0]), int(k)
        if S < 1 or S > 1 << 20:
            raise ValueError(f"plda_score_topk: S={S} speakers (1 .. 2^20)")
        self._plda_f64("plda_score_topk", "r", r, (S,))
        if k < 1 or k > 4:
            raise ValueError(f"plda_score_topk: k={k} (1 .. 4)")
        nbytes = int(self.lib.sdk_plda_score_workspace_bytes(N, S, k))
        if nbytes == 0:
            raise SdkError(f"sdk_plda_score_workspace_bytes: {self.lib.sdk_last_error().decode()}")
        dev = X.device
        if ws is None:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        elif ws.dtype != torch.uint8 or ws.dim() != 1 or not ws.is_cuda or not ws.is_contiguous():
            raise ValueError(f"plda_score_topk: ws must be a contiguous uint8 device tensor, got {tuple(ws.shape)} {ws.dtype}")
        idx = torch.empty((N, k), dtype=torch.int32, device=dev)
        sc = torch.empty((N, k), dtype=torch.float64, device=dev)
        full = torch.empty((N, S), dtype=torch.float64, device=dev) if scores else None
        check(self.lib.sdk_plda_score_topk(self.ctx, X.data_ptr(), N, D, G.data_ptr(), r.data_ptr(), S, k, idx.data_ptr(), sc.data_ptr(), _ptr(full),
                                           ws.data_ptr(), ws.numel(), _stream()), "sdk_plda_score_topk")
        return (idx, sc, full) if scores else (idx, sc)

    # ---- verification trials (trials.py; csrc/trials.hip): nothing here synchronises with the host
    def trial_hist(self, A: torch.Tensor, B: torch.Tensor, r: torch.Tensor, la: torch.Tensor, sa: torch.Tensor, lb: torch.Tensor,
                   sb: torch.Tensor, lo: float, hi: float, shift: int = 12, base: int = 0, max_blocks: int = 0):
        """One pass of the trial histogram: A [N, K] test rows, B [M, K] model rows, r [M] float64 (K a multiple of 16 in 16 .. 512,
        1 <= N, M <= 2^20), la, sa [N] and lb, sb [M] int32 labels and sessions, all on the device -> (hist [2, 4096], under [2], over [2],
        nan [2], excluded [1]) int64 device tensors, views of one array (sdk_trial_hist; trials.py states the rule).  The score
        r[j] + A[i] . B[j] is cut into q = floor((s - lo) * scale), scale = 2^24 / (hi - lo) formed here in float64, and lands in bin
        (q >> shift) - base.  max_blocks: 0 = the default grid, else a cap on the workgroups (the counts do not depend on it)."""
        self._plda_f64("trial_hist", "A", A, (None, None))
        N, K = int(A.shape[0]), int(A.shape[1])
        if K < 16 or K > 512 or K % 16:
            raise ValueError(f"trial_hist: K={K} not supported (a multiple of 16 in 16 .. 512)")
        self._plda_f64("trial_hist", "B", B, (None, K))
        M = int(B.shape[0])
        if not (1 <= N <= 1 << 20 and 1 <= M <= 1 << 20):
            raise ValueError(f"trial_hist: N={N} test rows, M={M} model rows (1 .. 2^20 each)")
        self._plda_f64("trial_hist", "r", r, (M,))
        for name, t, n in (("la", la, N), ("sa", sa, N), ("lb", lb, M), ("sb", sb, M)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (n,) or not t.is_contiguous() or not t.is_cuda:
                raise ValueError(f"trial_hist: {name} must be a contiguous int32 [{n}] device tensor, got "
                                 f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__} {getattr(t, 'dtype', '')}")
        lo, hi, shift, base, max_blocks = float(lo), float(hi), int(shift), int(base), int(max_blocks)
        if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
            raise ValueError(f"trial_hist: score range ({lo}, {hi}): finite lo < hi expected")
        with np.errstate(over="ignore"):
            scale = float(np.float64(16777216.0) / (np.float64(hi) - np.float64(lo)))
        if not (np.isfinite(scale) and scale > 0.0):
            raise ValueError(f"trial_hist: scale = 2^24 / (hi - lo) = {scale} is not a finite number above 0 (range ({lo}, {hi}))")
        if shift < 0 or shift > 24:
            raise ValueError(f"trial_hist: shift={shift} (0 .. 24)")
        if base < 0 or base > 1 << 24:
            raise ValueError(f"trial_hist: base={base} (0 .. 2^24)")
        if max_blocks < 0:
            raise ValueError(f"trial_hist: max_blocks={max_blocks} (0: the default grid, else a cap on the workgroups)")
        out = torch.empty((2 * 4096 + 7,), dtype=torch.int64, device=A.device)           # uint64 counters, all below 2^40
        check(self.lib.sdk_trial_hist(self.ctx, A.data_ptr(), N, B.data_ptr(), r.data_ptr(), M, K, la.data_ptr(), sa.data_ptr(), lb.data_ptr(),
                                      sb.data_ptr(), lo, scale, shift, base, max_blocks, out.data_ptr(), _stream()), "sdk_trial_hist")
        return out[:8192].view(2, 4096), out[8192:8194], out[8194:8196], out[8196:8198], out[8198:8199]

    # ---- spherical k-means on unit rows (cluster.kmeans_cluster; csrc/kmeans.hip): the whole loop in one enqueue, nothing read back here
    def kmeans_rows(self, E: torch.Tensor, rows: torch.Tensor, k: int, max_iters: int = 20, check_rows: bool = True):
        """E [R, d] fp32 unit rows, rows [n] int32 ascending (device), 1 <= k <= min(n, 64) -> (labels [n] int32 in [0, k), not canonical,
        n_iter [1] int32, status [1] int32), all on the device and not read back: sdk_kmeans_rows (the rule: cluster.kmeans_cluster).  The
        caller reads n_iter and status once.  check_rows=False: the caller has checked that rows lie in [0, R)."""
        n = self._vbx_rows("kmeans_rows", E, rows, check_rows)
        k, max_iters, d = int(k), int(max_iters), int(E.shape[1])
        if k < 1 or k > min(n, 64):
            raise ValueError(f"kmeans_rows: k={k} (1 .. min(n, 64), n={n})")
        if max_iters < 1 or max_iters > 1000:
            raise ValueError(f"kmeans_rows: max_iters={max_iters} (1 .. 1000)")
        nbytes = self.lib.sdk_kmeans_rows_workspace_bytes(n, d, k)
        if nbytes == 0:
            raise SdkError(f"sdk_kmeans_rows_workspace_bytes: {self.lib.sdk_last_error().decode()}")
        dev = E.device
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        labels = torch.empty((n,), dtype=torch.int32, device=dev)
        n_iter = torch.empty((1,), dtype=torch.int32, device=dev)
        status = torch.empty((1,), dtype=torch.int32, device=dev)
        check(self.lib.sdk_kmeans_rows(self.ctx, E.data_ptr(), rows.data_ptr(), n, d, k, max_iters, labels.data_ptr(), n_iter.data_ptr(),
                                       status.data_ptr(), ws.data_ptr(), nbytes, _stream()), "sdk_kmeans_rows")
        return labels, n_iter, status

    def asp_fused(self, ah, w2, b2, h, B, T, kblocked=False):
        """kblocked: h is [Cm / 64, B*T, 64] (to_kblocked) - the per-segment form only (sdk_asp_kblocked_ok).  The element format (bf16 or
        fp16) is h's dtype; ah and w2 must match it."""
        fmt = _elem_fmt(h, "asp_fused")
        if ah.dtype != h.dtype or w2.dtype != h.dtype:
            raise ValueError(f"asp_fused: ah {ah.dtype}, w2 {w2.dtype} and h {h.dtype} must share one element format")
        if kblocked:
            Cm = h.shape[0] * 64
            out = torch.empty((B, 2 * Cm), dtype=torch.float32, device=self.device)
            check(self.lib.sdk_asp_fused_kblocked_fmt(self.ctx, ah.data_ptr(), ah.stride(0), w2.data_ptr(), b2.data_ptr(), h.data_ptr(),
                                                      B, T, Cm, ah.shape[1], out.data_ptr(), fmt, _stream()), "sdk_asp_fused_kblocked_fmt")
            return out
        Cm = h.shape[1]
        out = torch.empty((B, 2 * Cm), dtype=torch.float32, device=self.device)
        check(self.lib.sdk_asp_fused_fmt(self.ctx, ah.data_ptr(), ah.stride(0), w2.data_ptr(), b2.data_ptr(), h.data_ptr(), h.stride(0),
                                         B, T, Cm, ah.shape[1], out.data_ptr(), fmt, _stream()), "sdk_asp_fused_fmt")
        return out


_engines: Dict[int, Engine] = {}


def get_engine(device: int = 0, **kw) -> Engine:
    if device not in _engines:
        _engines[device] = Engine(device, **kw)
    return _engines[device]
