"""tests/hp_ref.py on the CPU: the pair model against Engine.to_planes and its storage bound over fp16's whole range, the four sweep
restatements against oracle/ecapa.py, and each bound against an fp32 emulation of its kernel's summation order (inside) and against
the mistakes the GPU sweeps are there to catch (outside)."""
import numpy as np
import pytest
import torch

import hp_ref as H
from conftest import sub
from oracle import ecapa as oecapa

W = sub("weights")
OPS = sub("ops")


@pytest.fixture(scope="module")
def weights():
    return W.synthetic_weights(0)


def _magnitudes():
    """powers of two from 2^-30 to 2^15 with their fp32 neighbours, fp16's half-way points, the range's end and random fill"""
    p = 2.0 ** torch.arange(-30, 16, dtype=torch.float64)
    near = torch.cat([p, p * (1 + 2.0 ** -23), p * (1 - 2.0 ** -24), p * (1 + 2.0 ** -11), p * (1 + 2.0 ** -11 + 2.0 ** -23), p * (1 + 2.0 ** -12),
                      p * (1 + 2.0 ** -12 - 2.0 ** -23), p * 1.5, p * (2 - 2.0 ** -11), p * (2 - 2.0 ** -23)])
    g = torch.Generator().manual_seed(0)
    rnd = torch.exp2(torch.rand(200000, generator=g, dtype=torch.float64) * 46 - 30) * (1 + torch.rand(200000, generator=g, dtype=torch.float64))
    v = torch.cat([near, rnd, torch.tensor([65504.0, 65503.99, 65488.0, 65472.0, 0.0])]).float()
    v = v[v.abs() <= H.HP_MAX]
    return torch.cat([v, -v])


def test_split_is_to_planes_and_join_is_exact():
    v = _magnitudes()
    hi, lo = H.split(v)
    P = OPS.Engine.to_planes(v[:, None])
    assert torch.equal(P[:, 0].view(torch.int16), hi.view(torch.int16)) and torch.equal(P[:, 1].view(torch.int16), lo.view(torch.int16))
    # the kernels join in fp32: exact for a pair that split made, and what Engine.from_planes gives
    j32 = hi.float() + lo.float() * (1.0 / 2048.0)
    assert torch.equal(j32.double(), H.join(hi, lo)) and torch.equal(OPS.Engine.from_planes(P)[:, 0], j32)
    x = torch.randn(37, 24) * 5
    assert torch.equal(OPS.Engine.to_planes(x), torch.cat(H.split(x), 1))
    buf = H.planes(x, 64, 32, rows_extra=2)
    assert torch.equal(buf[:37, :24], H.split(x)[0]) and torch.equal(buf[:37, 32:56], H.split(x)[1])
    rest = torch.ones(39, 64, dtype=torch.bool)
    rest[:37, :24] = False
    rest[:37, 32:56] = False
    assert (buf[rest] == H.SENT).all() and float(H.join(torch.tensor(H.SENT).half(), torch.tensor(H.SENT).half())) == H.SENT * (1 + 1 / 2048)


def test_storage_bound_over_the_whole_range():
    v = _magnitudes()
    err = (H.decode(v) - v.double()).abs()
    bound = H.storage_bound(v)
    ratio = float((err / bound).max())
    print(f"pair storage: worst err / bound {ratio:.3f} over {v.numel()} values")
    assert (err <= bound).all(), ratio
    assert ratio > 0.2                      # the bound is the format's, not a loose one
    # 22 bits where both planes are normal, the 2^-36 floor below
    big = v.abs() >= 2.0 ** -3
    assert float((err[big] / v[big].abs().double()).max()) <= 2.0 ** -22
    assert float(err[v.abs() < 2.0 ** -14].max()) <= 2.0 ** -36
    # beyond the range: exactly +-65504, lo = 0 (no infinity, no NaN)
    over = torch.tensor([65504.0, 65505.0, 65520.0, 7e4, 1e9, 3.4e38, float("inf")])
    for s in (1.0, -1.0):
        hi, lo = H.split(over * s)
        assert (hi.double() == s * 65504.0).all() and (lo == 0).all()


# ---------------------------------------------------------------------------------------------------- against the oracle
def _oracle_z(orc, x, i):
    """z of SE-Res2Net block i, by the oracle's own layers (the first half of EcapaOracle.se_res2net)"""
    d = orc.dil[i - 1]
    u = orc.tdnn(x, f"blk{i}.tdnn1")
    s = u.shape[-1] // orc.scale
    ys, prev = [u[..., :s]], None
    for c in range(1, orc.scale):
        inp = u[..., c * s:(c + 1) * s] if c == 1 else u[..., c * s:(c + 1) * s] + prev
        prev = orc.tdnn(inp, f"blk{i}.res2net.{c - 1}", d)
        ys.append(prev)
    return orc.tdnn(torch.cat(ys, -1), f"blk{i}.tdnn2")


def test_mean_and_se_apply_reproduce_the_oracles_block(weights):
    orc = oecapa.EcapaOracle(weights, "fp32", torch.float64)
    B, T, C = 2, 11, 1024
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, T, C, generator=g)
    z = _oracle_z(orc, x, 1)
    want = orc.se_res2net(x, 1).double().reshape(B * T, C)
    mean, e_mean = H.seg_mean_ref(z.reshape(B * T, C), B, T)
    assert torch.equal(mean, z.double().mean(1)) and (e_mean > 0).all()
    w1, b1 = (torch.from_numpy(weights[f"blk1.se.conv1.{k}"]).double() for k in ("w", "b"))
    w2, b2 = (torch.from_numpy(weights[f"blk1.se.conv2.{k}"]).double() for k in ("w", "b"))
    gate = torch.sigmoid(torch.relu(mean @ w1[:, :, 0].T + b1) @ w2[:, :, 0].T + b2)
    tgt, bound, pre, acc = H.se_apply_ref(z.reshape(B * T, C), x.reshape(B * T, C), gate, B, T)
    assert torch.equal(tgt, pre)                                      # nothing saturates here
    # the oracle's gate and product are fp32: a few 2^-24 of the terms; a wrong mean, gate row or residual is 1e-2 away
    err = (pre - want).abs()
    assert (err <= 8 * acc + 1e-12).all(), float((err / acc.clamp_min(1e-300)).max())
    assert (bound >= acc + H.storage_bound(tgt)).all()
    wrong = H.se_apply_ref(z.reshape(B * T, C), x.reshape(B * T, C), gate.roll(1, 0), B, T)[2]
    assert float(((wrong - want).abs() / bound).max()) > 1e3


def test_asp_stages_reproduce_the_oracles_pooling(weights):
    orc = oecapa.EcapaOracle(weights, "fp32", torch.float64)
    g = torch.Generator().manual_seed(3)
    B, T = 2, 12
    _, inter = orc.forward_pooled(torch.randn(B, T, 80, generator=g) * 3)
    h = inter["mfa"].reshape(B * T, -1).double()
    Cm = h.shape[1]
    # stage 1, the global context: through the attention's hidden layer, which is what the oracle keeps of it
    ctx, e_ctx = H.asp_stats_ref(h, B, T)
    Wt = torch.from_numpy(weights["asp.tdnn.conv.w"][:, :, 0]).double()
    ubias = ctx @ Wt[:, Cm:].T + torch.from_numpy(weights["asp.tdnn.conv.b"]).double()
    s, sh = orc.bn("asp.tdnn.bn")
    a = torch.tanh(torch.relu((h @ Wt[:, :Cm].T).reshape(B, T, -1) + ubias[:, None]) * s.double() + sh.double())
    assert float((a - inter["attn_hidden"].double()).abs().max()) < 1e-5
    sd, mu = torch.std_mean(h.reshape(B, T, -1), 1, correction=0)
    assert torch.allclose(ctx, torch.cat([mu, sd.clamp_min(1e-6)], 1), rtol=1e-12, atol=1e-12) and (e_ctx > 0).all()
    # stage 2, the pooling, on the oracle's own fp32 logits
    logits = ((inter["attn_hidden"].double() @ torch.from_numpy(weights["asp.conv.w"][:, :, 0]).double().T).float() + torch.from_numpy(weights["asp.conv.b"]))
    got, err = H.asp_pool_ref(logits.reshape(B * T, Cm), h, B, T)
    want = inter["pooled"].double()
    assert ((got - want).abs() <= err + 2 * H.EPS32 * want.abs()).all()        # the oracle's pooled is fp32
    wrong, _ = H.asp_pool_ref(logits.reshape(B * T, Cm).roll(1, 0), h, B, T)
    assert float(((wrong - want).abs() / err).max()) > 1e3


# ---------------------------------------------------------------------------------------------------- the bounds against fp32 emulations
f32 = np.float32


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _emul_seg_mean(z, T, drop_last=False):
    s = [np.zeros(z.shape[1:], f32) for _ in range(4)]
    for t in range(T - 1 if drop_last else T):
        s[t % 4] = (s[t % 4] + z[t]).astype(f32)
    return ((((s[0] + s[1]).astype(f32) + s[2]).astype(f32) + s[3]).astype(f32) * (f32(1.0) / f32(T))).astype(f32)


def _emul_stats(h, T):
    K = h[0]
    s1 = [np.zeros_like(K), np.zeros_like(K)]
    s2 = [np.zeros_like(K), np.zeros_like(K)]
    for t in range(T):
        d = (h[t] - K).astype(f32)
        s1[t % 2] = (s1[t % 2] + d).astype(f32)
        s2[t % 2] = _fma(d, d, s2[t % 2])
    invT = f32(1.0) / f32(T)
    a = ((s1[0] + s1[1]).astype(f32) * invT).astype(f32)
    q = ((s2[0] + s2[1]).astype(f32) * invT).astype(f32)
    return np.concatenate([(K + a).astype(f32), np.sqrt(np.maximum(_fma(-a, a, q), f32(1e-12))).astype(f32)])


def _emul_pool(lg, h, T, skip_rescale_at=None):
    K = h[0]
    mx = np.full_like(K, -np.inf)
    se, s1, s2 = np.zeros_like(K), np.zeros_like(K), np.zeros_like(K)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            l = lg[t]
            d = (h[t] - K).astype(f32)
            grow = l > mx
            r = np.where(grow, np.exp((mx - l).astype(f32)).astype(f32), f32(1.0)).astype(f32)
            if skip_rescale_at == t:
                r = np.ones_like(r)
            se, s1, s2 = (se * r).astype(f32), (s1 * r).astype(f32), (s2 * r).astype(f32)
            mx = np.where(grow, l, mx)
            w = np.exp((l - mx).astype(f32)).astype(f32)
            se = (se + w).astype(f32)
            s1 = _fma(w, d, s1)
            s2 = _fma((w * d).astype(f32), d, s2)
    a, q = (s1 / se).astype(f32), (s2 / se).astype(f32)
    return np.concatenate([(K + a).astype(f32), np.sqrt(np.maximum(_fma(-a, a, q), f32(1e-12))).astype(f32)])


def _ratio(got, want, bound):
    err = (torch.from_numpy(np.asarray(got)).double() - want).abs()
    assert not torch.isnan(err).any()
    return float((err / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 201, 501])
def test_bounds_hold_for_an_fp32_emulation_of_each_kernel(T):
    """the kernels' summation orders in numpy fp32, one segment of 64 channels: inside the bounds, and not by orders of magnitude"""
    g = torch.Generator().manual_seed(T)
    C = 64
    h = H.decode(torch.randn(T, C, generator=g) * 2 + 3)
    h[:, :4] = H.decode(torch.tensor(2.5))                                   # constant columns: the variance floor
    if T > 1:
        h[0, 4:8] = H.decode(torch.tensor(100.0))                            # a transient frame 0
        h[1:, 4:8] = H.decode(torch.randn(T - 1, 4, generator=g) * 0.01)
    hn = h.numpy().astype(f32)
    assert np.array_equal(hn.astype(np.float64), h.numpy())
    want, bound = H.seg_mean_ref(h, 1, T)
    r_mean = _ratio(_emul_seg_mean(hn, T), want[0], bound[0])
    want, bound = H.asp_stats_ref(h, 1, T)
    r_stats = _ratio(_emul_stats(hn, T), want[0], bound[0])
    r_pool = 0.0
    t = torch.arange(T, dtype=torch.float32)[:, None].expand(T, C)
    kinds = {"normal": torch.randn(T, C, generator=g) * 3, "ascending": t * 0.05 + torch.rand(1, C, generator=g),
             "descending": -t * 0.05, "equal": torch.full((T, C), 1.5), "offset": torch.randn(T, C, generator=g) * 3 + 1e4}
    for kind, lg in kinds.items():
        lg = lg.contiguous()
        want, bound = H.asp_pool_ref(lg, h, 1, T)
        r = _ratio(_emul_pool(lg.numpy(), hn, T), want[0], bound[0])
        assert r <= 1.0, (kind, r)
        r_pool = max(r_pool, r)
        if kind == "ascending":
            assert float(H.rescales_after(lg.double()[None])[0, 0].min()) == T - 1
        if kind in ("descending", "equal"):
            assert float(H.rescales_after(lg.double()[None]).max()) == 0
    print(f"T {T}: emulated seg_mean {r_mean:.3f} asp_stats {r_stats:.3f} asp_pool {r_pool:.3f} of the bound")
    assert r_mean <= 1.0 and r_stats <= 1.0


def test_bounds_catch_the_mistakes_they_are_for():
    """a dropped last frame, a neighbouring channel block, a missed rescale: each far outside the bound"""
    g = torch.Generator().manual_seed(5)
    T, C = 201, 64
    h = H.decode(torch.randn(T, C, generator=g) * 2 + 3)
    hn = h.numpy().astype(f32)
    want, bound = H.seg_mean_ref(h, 1, T)
    assert _ratio(_emul_seg_mean(hn, T, drop_last=True), want[0], bound[0]) > 100
    assert _ratio(np.roll(_emul_seg_mean(hn, T), 8), want[0], bound[0]) > 100
    lg = (torch.arange(T, dtype=torch.float32)[:, None] * 0.05).expand(T, C).contiguous()
    want, bound = H.asp_pool_ref(lg, h, 1, T)
    assert _ratio(_emul_pool(lg.numpy(), hn, T), want[0], bound[0]) <= 1.0
    assert _ratio(_emul_pool(lg.numpy(), hn, T, skip_rescale_at=T - 3), want[0], bound[0]) > 100
    # se_apply: one storage step of the pair (2^-22) is already outside
    z, x = H.decode(torch.randn(T, C, generator=g)), H.decode(torch.randn(T, C, generator=g))
    gate = torch.rand(1, C, generator=g)
    tgt, bnd, _, _ = H.se_apply_ref(z, x, gate, 1, T)
    assert float(((tgt * (1 + 2.0 ** -20) - tgt).abs() / bnd).max()) > 1.0
