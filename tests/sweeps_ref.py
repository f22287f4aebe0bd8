"""float64 restatements of the per-utterance sweeps (csrc/pool_se.hip) and of the fused Res2Net chain (csrc/res2net.hip) for
tests/test_ecapa_sweeps.py.  Every function takes the STORED 2-byte inputs (as float64) and rounds to the storage format only where the
kernel stores: fmt 0 = bf16, fmt 2 = fp16 (the C ABI's `precision` argument), fp16 saturating at +-65504 and keeping NaN as the kernels do.
Each returns the exact value and a bound on the kernel's fp32 error next to it: n 2^-24 sum|terms| for a sum of n terms, plus the error
its inputs carry in from earlier fp32 steps.  tests/test_sweeps_ref_cpu.py checks these against oracle/ecapa.py."""
import torch

from oracle import ecapa as oecapa

EPS32 = 2.0 ** -24
FP16_MAX = 65504.0
STD_EPS = 1e-12
FMTS = {0: torch.bfloat16, 2: torch.float16}
BITS = {0: 8, 2: 11}


def store(x, fmt):
    """float64 -> the 2-byte storage format (round to nearest even) -> float64; fp16 saturates finite overflow at +-65504, NaN stays NaN"""
    x = torch.as_tensor(x, dtype=torch.float64)
    if fmt == 2:
        x = torch.where(torch.isnan(x), x, x.clamp(-FP16_MAX, FP16_MAX))
    return x.float().to(FMTS[fmt]).double()


def ulp(x, fmt):
    """spacing of the storage format at |x| (fp16 below 2^-14: the subnormal spacing 2^-24)"""
    a = torch.as_tensor(x, dtype=torch.float64).abs().clamp_min(1e-300)
    e = torch.floor(torch.log2(a))
    if fmt == 2:
        e = e.clamp_min(-14.0)
    return torch.pow(2.0, e - (BITS[fmt] - 1))


def stored_bound(want, acc, fmt):
    """(target, bound) for a stored output: the saturated exact value, one storage ulp of it plus the fp32 error `acc`"""
    w = want if fmt != 2 else torch.where(torch.isnan(want), want, want.clamp(-FP16_MAX, FP16_MAX))
    return w, ulp(w, fmt) + acc


def sqrt_bound(var, e_var):
    """|sqrt(a) - sqrt(b)| <= |a - b| / max(sqrt(b), sqrt|a - b|), b = max(var, 1e-12), plus the rounding of the square root"""
    sd = var.clamp_min(STD_EPS).sqrt()
    return e_var / torch.maximum(sd, e_var.sqrt()).clamp_min(1e-300) + 2 * EPS32 * sd


# ---------------------------------------------------------------------------------------------------- squeeze-excitation
def se_ref(z, x, w1t, b1, w2t, b2, B, T):
    """out = fmt(g * z + x), g = sigmoid(FC2(relu(FC1(mean_t z)))).  z, x [B*T, C] stored values; w1t [C, Cse], w2t [Cse, C] fp32.
    Returns (pre-store value, fp32 error bound) [B*T, C]: the gate's error from the mean (T terms), FC1 (C), FC2 (Cse) and the sigmoid
    (__expf; sigmoid' <= 1/4), times |z|, plus the rounding of g * z + x."""
    C = z.shape[1]
    Cse = w1t.shape[1]
    zb, xb = z.double().reshape(B, T, C), x.double().reshape(B, T, C)
    w1t, b1, w2t, b2 = (t.double() for t in (w1t, b1, w2t, b2))
    mean = zb.mean(1)
    hid = torch.relu(mean @ w1t + b1)
    a = hid @ w2t + b2
    g = torch.sigmoid(a)
    want = g[:, None, :] * zb + xb
    d_mean = (T + 2) * EPS32 * zb.abs().mean(1)
    d_hid = (C + 2) * EPS32 * (mean.abs() @ w1t.abs() + b1.abs()) + d_mean @ w1t.abs()
    d_a = (Cse + 2) * EPS32 * (hid @ w2t.abs() + b2.abs()) + d_hid @ w2t.abs()
    d_g = d_a / 4 + (a.abs() + 8) * EPS32
    acc = d_g[:, None, :] * zb.abs() + 2 * EPS32 * ((g[:, None, :] * zb).abs() + xb.abs())
    return want.reshape(B * T, C), acc.reshape(B * T, C)


# ---------------------------------------------------------------------------------------------------- attentive statistics pooling
def asp_stats_ref(h, B, T):
    """[B, 2C] mean | sqrt(max(var, 1e-12)) over frames, and its bound: the kernel sums about K = h[t = 0] in fp32, so the rounding follows
    the shifted terms (|h - K| <= |h - mu| + |K - mu|, and (K - mu)^2 <= T var: a bounded loss)"""
    C = h.shape[1]
    hb = h.double().reshape(B, T, C)
    mu = hb.mean(1)
    var = ((hb - mu[:, None]) ** 2).mean(1)
    d = hb - hb[:, :1]
    e_mu = (T + 4) * EPS32 * d.abs().mean(1) + 2 * EPS32 * mu.abs()
    e_var = 3 * (T + 4) * EPS32 * (d ** 2).mean(1)
    return torch.cat([mu, var.clamp_min(STD_EPS).sqrt()], 1), torch.cat([e_mu, sqrt_bound(var, e_var)], 1)


def asp_pool_ref(logits, h, B, T, d_logit=None):
    """softmax over frames of fp32 logits [B*T, C] -> weighted mean | std of h [B, 2C], and the bound.  A weight's relative error: the exp
    argument rounded in fp32 (max-subtraction, * log2 e, the online max) plus twice the largest error of the logits themselves (d_logit,
    [B*T, C]: the fused GEMM's); it moves the mean by sum w dw |h - mu| and the variance by sum w dw |(h - mu)^2 - var|.  Sums: n = T + 32
    (frames plus the per-tile merges of the per-segment kernel)."""
    C = h.shape[1]
    lg = logits.double().reshape(B, T, C)
    hb = h.double().reshape(B, T, C)
    w = torch.softmax(lg, 1)
    mu = (w * hb).sum(1)
    dev = hb - mu[:, None]
    var = (w * dev ** 2).sum(1)
    mx = lg.max(1, keepdim=True).values
    dw = 3 * EPS32 * (lg.abs() + mx.abs()) + 4 * EPS32
    if d_logit is not None:
        dw = dw + 2 * d_logit.double().reshape(B, T, C).amax(1, keepdim=True)
    n = T + 32
    e_mu = (w * dw * dev.abs()).sum(1) + n * EPS32 * (w * hb.abs()).sum(1) + 16 * EPS32 * hb.abs().amax(1)
    e_var = (w * dw * (dev ** 2 - var[:, None]).abs()).sum(1) + 2 * n * EPS32 * var + e_mu ** 2
    return torch.cat([mu, var.clamp_min(STD_EPS).sqrt()], 1), torch.cat([e_mu, sqrt_bound(var, e_var)], 1)


def asp_fused_ref(ah, w2, b2, h, B, T):
    """logits = ah w2^T + b2 (fp32 MFMA accumulation over A = 128), then asp_pool_ref"""
    ahd, w2d = ah.double(), w2.double()
    logits = ahd @ w2d.T + b2.double()
    d_logit = (w2d.shape[1] + 2) * EPS32 * (ahd.abs() @ w2d.abs().T)
    return asp_pool_ref(logits, h, B, T, d_logit)


# ---------------------------------------------------------------------------------------------------- Res2Net chain
def tdnn_ref(s, W, bias, scale, shift, T, dil):
    """one chain conv on stored inputs s [B*T, 128]: relu(k3 dilated conv with segment-local reflection + bias) * scale + shift.
    W [128, 3*128] tap-major.  Returns (pre-store value, fp32 error bound) [B*T, 128]."""
    M = s.shape[0]
    sb = s.double().reshape(M // T, T, -1)
    Wd = W.double()
    acc = torch.zeros(M // T, T, Wd.shape[0], dtype=torch.float64)
    mag = torch.zeros_like(acc)
    t = torch.arange(T)
    for j in range(3):
        src = oecapa.reflect_index(t + (j - 1) * dil, T)
        Wj = Wd[:, j * 128:(j + 1) * 128]
        acc += sb[:, src, :] @ Wj.T
        mag += sb[:, src, :].abs() @ Wj.abs().T
    r = torch.relu(acc + bias.double())
    y = r * scale.double() + shift.double()
    err = scale.double().abs() * (386 * EPS32 * mag + EPS32 * (acc + bias.double()).abs()) + 3 * EPS32 * (r * scale.double()).abs() + EPS32 * shift.double().abs()
    return y.reshape(M, -1), err.reshape(M, -1)


def chain_input(u, y_prev, fmt):
    """the running sum fmt(u_c + y_{c-1}) as the kernel forms it: one fp32 add of two stored values, then the store"""
    return store((u.float() + y_prev.float()).double(), fmt)


def res2net_chain_ref(U, W, bias, scale, shift, nconv, T, dil, fmt, exact=False):
    """the whole chain on U [B*T, >= 128 (nconv + 1)]: returns [y_1 .. y_nconv] stored.  exact: every value the kernel stores must be
    representable (integer / dyadic sweeps) - asserted, so that a bit-exact comparison is a comparison with float64"""
    ys = []
    prev = None
    for c in range(1, nconv + 1):
        u = U[:, 128 * c:128 * (c + 1)].double()
        s = u if c == 1 else chain_input(u, prev, fmt)
        if exact and c > 1:
            assert torch.equal(s, u + prev), "running sum not representable"
        y, _ = tdnn_ref(s, W[c - 1], bias[c - 1], scale[c - 1], shift[c - 1], T, dil)
        prev = store(y, fmt)
        if exact:
            assert torch.equal(prev, y), f"conv {c} output not representable in format {fmt}"
        ys.append(prev)
    return ys


def integer_chain_case(B, T, nconv, fmt, seed):
    """operands of an exact chain sweep: U small integers, each output row of W one +-1 at a random (tap, input) position (anywhere in the
    384-long k range), integer bias and shift, scale 1: every product, sum and stored value is an integer below 256 in magnitude, exact in
    both formats (res2net_chain_ref(exact=True) checks it).  Accumulation itself is covered by the real-valued sweeps."""
    g = torch.Generator().manual_seed(seed)
    U = torch.randint(-2, 3, (B * T, 128 * (nconv + 1)), generator=g).double()
    W = []
    for _ in range(nconv):
        Wc = torch.zeros(128, 384, dtype=torch.float64)
        Wc[torch.arange(128), torch.randint(0, 384, (128,), generator=g)] = torch.randint(0, 2, (128,), generator=g).double() * 2 - 1
        W.append(Wc)
    bias = [torch.randint(-2, 3, (128,), generator=g).double() for _ in range(nconv)]
    scale = [torch.ones(128, dtype=torch.float64) for _ in range(nconv)]
    shift = [torch.randint(-2, 3, (128,), generator=g).double() for _ in range(nconv)]
    return U, W, bias, scale, shift
