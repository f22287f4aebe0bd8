"""float64 restatements of the masked attentive statistics pooling (csrc/asp_masked.hip; the rule is in include/sdk_hip.h) for
tests/test_asp_masked_cpu.py and tests/test_asp_masked_gpu.py, following tests/sweeps_ref.py: every function takes the STORED 2-byte inputs
(as float64) and returns the exact value with a bound on the kernel's fp32 error next to it, n 2^-24 sum|terms| for the kernel's reduction.

The kernels' reduction: a thread sums its ceil(T / 4) frames in order, the four frame groups meet as (0 + 1) + (2 + 3), one division.  A
sum of k terms in any order errs by at most (k - 1) 2^-24 sum|terms| to first order; n = T + 8 below covers the longest chain
(ceil(T / 4) + 2 additions), the rounding of every term (the product w h is fused; h - mu and its square round once each) and of v1 (the
same chain over the weights), with room, as sweeps_ref's T + 4 does for the unmasked kernel.

MaskedEcapaOracle: oracle.ecapa.EcapaOracle with the pooling replaced by the masked rule (S weight rows per segment); the trunk is the
parent's, line for line, and acc = torch.float32 / float64 is honoured in every GEMM as the parent does."""
import torch

from oracle import ecapa as oecapa
from sweeps_ref import EPS32, STD_EPS, sqrt_bound


def asp_stats_masked_ref(h, w, B, T):
    """h [B*T, C] stored values, w [B, S, T] >= 0 -> ([B*S, 2C] mean | sqrt(max(var, 1e-12)), bound).  n = T + 8 (module docstring).
    mean: the kernel sums w h (no shift), so the bound follows sum w |h| / v1; variance: two passes, a sum of non-negative terms about the
    ROUNDED mean mu': sum w (h - mu')^2 / v1 = var + (mu - mu')^2 exactly, hence e_mu^2.  Rows without weight (v1 <= 0) are zeros."""
    C = h.shape[1]
    S = w.shape[1]
    hb = h.double().reshape(B, 1, T, C)
    wd = w.double().reshape(B, S, T, 1)
    v1 = wd.sum(2)                                                      # [B, S, 1]
    ok = v1 > 0
    v1s = torch.where(ok, v1, torch.ones_like(v1))
    mu = (wd * hb).sum(2) / v1s
    dev = hb - mu[:, :, None]
    var = (wd * dev ** 2).sum(2) / v1s
    n = T + 8
    e_mu = n * EPS32 * (wd * hb.abs()).sum(2) / v1s + 2 * EPS32 * mu.abs()
    e_var = 3 * n * EPS32 * var + e_mu ** 2
    want = torch.cat([mu, var.clamp_min(STD_EPS).sqrt()], -1)
    bound = torch.cat([e_mu, sqrt_bound(var, e_var)], -1)
    okk = ok.expand(B, S, 2 * C)
    return torch.where(okk, want, torch.zeros_like(want)).reshape(B * S, 2 * C), torch.where(okk, bound, torch.zeros_like(bound)).reshape(B * S, 2 * C)


def asp_pool_masked_ref(logits, h, w, B, T):
    """fp32 logits [B*T, C] of ONE slot, h [B*T, C] stored values, w [B, T] >= 0 -> ([B, 2C] weighted mean | std, bound): softmax over the
    frames with w > 0 (the others enter nothing - their logits may be NaN or inf), e = w exp(l - m), alpha = e / sum e.  A weight's relative
    error dw: the exp argument rounded in fp32 (max-subtraction, * log2 e: 3 2^-24 (|l| + |m|)), __expf and the product with w (5 2^-24).
    n = T + 8 (module docstring); the mean is s1 / l (both sums err: 2 n), the variance s2 / l about the rounded mean.  Rows without an
    active frame are zeros."""
    C = h.shape[1]
    lg = logits.double().reshape(B, T, C)
    hb = h.double().reshape(B, T, C)
    wd = w.double().reshape(B, T, 1)
    act = (wd > 0).expand(B, T, C)
    lgm = torch.where(act, lg, torch.full_like(lg, -float("inf")))
    mx = lgm.max(1, keepdim=True).values
    ok = torch.isfinite(mx)
    mxs = torch.where(ok, mx, torch.zeros_like(mx))
    lga = torch.where(act, lg, mxs.expand(B, T, C))
    e = torch.where(act, wd * torch.exp(lga - mxs), torch.zeros_like(lg))
    l = e.sum(1, keepdim=True)
    al = e / torch.where(l > 0, l, torch.ones_like(l))
    mu = (al * hb).sum(1)
    dev = hb - mu[:, None]
    var = (al * dev ** 2).sum(1)
    dw = 3 * EPS32 * (lga.abs() + mxs.abs()) + 5 * EPS32
    n = T + 8
    e_mu = (al * dw * dev.abs()).sum(1) + 2 * n * EPS32 * (al * hb.abs()).sum(1) + 2 * EPS32 * mu.abs()
    e_var = (al * dw * (dev ** 2 - var[:, None]).abs()).sum(1) + 3 * n * EPS32 * var + e_mu ** 2
    want = torch.cat([mu, var.clamp_min(STD_EPS).sqrt()], 1)
    bound = torch.cat([e_mu, sqrt_bound(var, e_var)], 1)
    okk = torch.cat([ok[:, 0], ok[:, 0]], 1)
    return torch.where(okk, want, torch.zeros_like(want)), torch.where(okk, bound, torch.zeros_like(bound))


class MaskedEcapaOracle(oecapa.EcapaOracle):
    """EcapaOracle with S masked poolings per segment.  forward_pooled(feats) keeps the parent's meaning (all-ones weights, S = 1);
    forward_pooled_masked(feats, w [B, S, T]) -> pooled [B, S, 2 Cm]; embed_masked -> raw embeddings [B, S, embed_dim] (rows without weight: zeros)."""

    def trunk(self, feats):
        """The parent's forward_pooled up to h, line for line."""
        inter = {}
        x0 = self.q(feats, "feats")
        x = self.q(self.tdnn(x0, "blk0"), "blk0")
        inter["blk0"] = x
        outs = []
        for i in range(1, len(self.dil) + 1):
            x = self.se_res2net(x, i)
            inter[f"blk{i}"] = x
            outs.append(x)
        cat = torch.cat(outs, dim=-1)
        h = self.q(self.tdnn(cat, "mfa"), "mfa")
        inter["mfa"] = h
        return h, inter

    def pool_masked(self, h, w, as64=False):
        """h [B, T, Cm] (stored), w [B, S, T] -> pooled [B, S, 2 Cm] fp32, in float64 where the parent's pooling is.  as64: the float64
        values before the fp32 store (the parent stores fp32 too), for comparisons tighter than an fp32 ulp."""
        B, T, Cm = h.shape
        S = w.shape[1]
        hd = h.double()
        Wt = self.w["asp.tdnn.conv.w"][:, :, 0]
        Wh = self.qw(Wt[:, :Cm], "asp").to(self.acc)
        W2 = self.qw(self.w["asp.conv.w"][:, :, 0], "asp").to(self.acc)
        s, sh = self.bn("asp.tdnn.bn")
        hW = (h.to(self.acc) @ Wh.T).float()                                   # [B, T, A]: shared by the slots
        out = torch.zeros(B, S, 2 * Cm, dtype=torch.float64 if as64 else torch.float32)
        for k in range(S):
            wd = w[:, k].double()                                            # [B, T]
            v1 = wd.sum(1)
            for b in range(B):
                if not v1[b] > 0:
                    continue
                wb = wd[b][:, None]
                mu = (wb * hd[b]).sum(0) / v1[b]
                sd = torch.sqrt(((wb * (hd[b] - mu) ** 2).sum(0) / v1[b]).clamp_min(oecapa.STD_EPS))
                ctx = torch.cat([mu, sd]).float()
                ubias = (ctx.double() @ Wt[:, Cm:].double().T).float() + self.w["asp.tdnn.conv.b"]
                a = self.q(torch.tanh(torch.relu(hW[b] + ubias) * s + sh), "attn_hidden")
                logits = (a.to(self.acc) @ W2.T).float() + self.w["asp.conv.b"]
                act = wd[b] > 0
                lg = logits.double()[act]
                e = wd[b][act][:, None] * torch.exp(lg - lg.max(0).values)
                al = e / e.sum(0)
                wmu = (al * hd[b][act]).sum(0)
                wsd = torch.sqrt((al * (hd[b][act] - wmu) ** 2).sum(0).clamp_min(oecapa.STD_EPS))
                out[b, k] = torch.cat([wmu, wsd]).to(out.dtype)
        return out

    def forward_pooled_masked(self, feats, w):
        h, inter = self.trunk(feats)
        pooled = self.pool_masked(h, torch.as_tensor(w))
        inter["pooled"] = pooled
        return pooled, inter

    def forward_pooled(self, feats):
        pooled, inter = self.forward_pooled_masked(feats, torch.ones(feats.shape[0], 1, feats.shape[1]))
        inter["pooled"] = pooled[:, 0]
        return pooled[:, 0], inter

    def embed_masked(self, feats, w):
        feats = torch.as_tensor(feats, dtype=torch.float32)
        w = torch.as_tensor(w)
        pooled, _ = self.forward_pooled_masked(feats, w)
        s, sh = self.bn("asp_bn")
        p = pooled * s + sh
        emb = (p.double() @ self.w["fc.w"][:, :, 0].double().T).float() + self.w["fc.b"]
        return torch.where((w.double().sum(-1) > 0)[..., None], emb, torch.zeros_like(emb))
