"""Engine's building blocks, kept for tests and tuning: the conv GEMM of both modes, the layout conversions, and the sweeps of the forward
one kernel at a time (SE, attentive statistics pooling, the per-utterance FC).  The product's forward never calls them: it is one C call.

BlocksMixin is a mixin of ops.Engine: no state and no __init__ of its own.  It uses self.lib, self.ctx, self.device, self._workspace
only, and this module imports ops.py for nothing (ops.py imports it).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import ConvGemmArgs, check
from .ops_util import _elem_fmt, _need, _ptr, _stream


class BlocksMixin:
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

    # ---- the single-plane sweeps (csrc/pool_se.hip); the element format (bf16 or fp16) is the activations' dtype
    def se_gate_residual(self, z, x, w1t, b1, w2t, b2, B, T, split: bool = True):
        C_ = z.shape[1]
        out = torch.empty_like(z)
        ws = self._workspace("sdk_se_workspace_bytes", B, C_, w1t.shape[1], cache="se") if split else None
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
