"""tests/sweeps_ref.py against oracle/ecapa.py on the same values (no GPU): the Res2Net chain, SE and ASP restatements that
tests/test_ecapa_sweeps.py judges the kernels by must reproduce the oracle's block and pooling, so a wrong reference fails here."""
import numpy as np
import pytest
import torch

import sweeps_ref as R
from conftest import sub
from oracle import ecapa as oecapa

W = sub("weights")


@pytest.fixture(scope="module")
def weights():
    return W.synthetic_weights(0)


def test_store_models_the_kernels_rounding():
    x = torch.tensor([1.0 + 2 ** -12, 1e6, -1e6, float("nan"), 3e-6, 2 ** -24 * 0.75, 65519.0, 65520.0])
    f = R.store(x, 2)
    assert f[0] == 1.0 and f[1] == 65504.0 and f[2] == -65504.0 and torch.isnan(f[3])
    assert f[4] == torch.tensor(3e-6).half().double() and f[5] == 2 ** -24 and f[6] == 65504.0 and f[7] == 65504.0
    b = R.store(x, 0)
    assert b[0] == 1.0 and b[1] == torch.tensor(1e6).bfloat16().double() and torch.isnan(b[3])
    assert float(R.ulp(1.5, 0)) == 2 ** -7 and float(R.ulp(1.5, 2)) == 2 ** -10 and float(R.ulp(1e-6, 2)) == 2 ** -24


def test_tdnn_ref_is_the_oracles_tdnn(weights):
    orc = oecapa.EcapaOracle(weights, "fp32", torch.float64)
    B, T, dil = 2, 17, 3
    g = torch.Generator().manual_seed(0)
    x = R.store(torch.randn(B * T, 128, generator=g), 0)
    name = "blk1.res2net.2"
    want = orc.tdnn(x.float().reshape(B, T, 128), name, dil).double().reshape(B * T, 128)
    Wk = torch.from_numpy(weights[f"{name}.conv.w"]).double()
    Wt = torch.cat([Wk[:, :, j] for j in range(3)], 1)
    s, sh = orc.bn(f"{name}.bn")
    got, err = R.tdnn_ref(x, Wt, torch.from_numpy(weights[f"{name}.conv.b"]), s, sh, T, dil)
    # the oracle's fp32 epilogue differs from float64 by far less than the bound the GPU is judged by
    assert ((got - want).abs() <= err).all(), float((got - want).abs().max())


@pytest.mark.parametrize("fmt,bits", [(0, 8), (2, 11)])
def test_chain_and_se_ref_reproduce_the_oracles_block(weights, fmt, bits):
    """one SE-Res2Net block of the oracle (rounding sites tdnn1 / res2net / tdnn2 / se_out at the format's width) against
    res2net_chain_ref + se_ref on the oracle's own stored u and z"""
    sites = {s: bits for s in ("tdnn1", "res2net", "tdnn2", "se_out")}
    orc = oecapa.EcapaOracle(weights, "fp32", torch.float64, sites=sites)
    B, T = 2, 23
    g = torch.Generator().manual_seed(fmt)
    x = R.store(torch.randn(B, T, 1024, generator=g), fmt).float()
    want = orc.se_res2net(x, 1).double().reshape(B * T, 1024)
    u = orc.q(orc.tdnn(x, "blk1.tdnn1"), "tdnn1").reshape(B * T, 1024)
    Ws, bs, ss, hs = [], [], [], []
    for c in range(7):
        name = f"blk1.res2net.{c}"
        Wk = torch.from_numpy(weights[f"{name}.conv.w"]).double()
        Ws.append(torch.cat([Wk[:, :, j] for j in range(3)], 1))
        bs.append(torch.from_numpy(weights[f"{name}.conv.b"]))
        s, sh = orc.bn(f"{name}.bn")
        ss.append(s)
        hs.append(sh)
    ys = R.res2net_chain_ref(u.double(), Ws, bs, ss, hs, 7, T, orc.dil[0], fmt)
    r = torch.cat([u[:, :128].double()] + ys, 1)
    z = orc.q(orc.tdnn(r.float().reshape(B, T, 1024), "blk1.tdnn2"), "tdnn2").reshape(B * T, 1024)
    w1t = torch.from_numpy(weights["blk1.se.conv1.w"][:, :, 0]).T.contiguous()
    w2t = torch.from_numpy(weights["blk1.se.conv2.w"][:, :, 0]).T.contiguous()
    out, acc = R.se_ref(z.double(), x.reshape(B * T, 1024).double(), w1t, torch.from_numpy(weights["blk1.se.conv1.b"]), w2t,
                        torch.from_numpy(weights["blk1.se.conv2.b"]), B, T)
    got = R.store(out, fmt)
    # the oracle rounds fp32 values, the reference float64 ones: a stored value of the chain may flip by one ulp next to a rounding boundary,
    # and tdnn2 spreads a flip over every channel of its frame - measured 97 % of the outputs identical, the rest within 2^-(bits - 2) of the
    # block's scale.  A wrong tap, reflection or running sum moves most outputs by far more.
    assert float((got == want).double().mean()) > 0.95
    assert float((got - want).abs().max()) <= 2.0 ** -(bits - 2) * float(want.abs().max())


def test_asp_refs_reproduce_the_oracles_pooling(weights):
    orc = oecapa.EcapaOracle(weights, "bf16", torch.float64)
    g = torch.Generator().manual_seed(3)
    B, T = 2, 12
    _, inter = orc.forward_pooled(torch.randn(B, T, 80, generator=g) * 3)
    h = inter["mfa"].reshape(B * T, -1).double()
    a = inter["attn_hidden"].reshape(B * T, -1).double()
    W2 = R.store(torch.from_numpy(weights["asp.conv.w"][:, :, 0]), 0)
    got, err = R.asp_fused_ref(a, W2, torch.from_numpy(weights["asp.conv.b"]), h, B, T)
    want = inter["pooled"].double()
    assert ((got - want).abs() <= err + 2 * R.EPS32 * want.abs()).all()        # the oracle's pooled is fp32
    st, _ = R.asp_stats_ref(h, B, T)
    sd, mu = torch.std_mean(h.reshape(B, T, -1), 1, correction=0)
    assert torch.allclose(st, torch.cat([mu, sd.clamp_min(1e-6)], 1), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("fmt", [0, 2])
@pytest.mark.parametrize("nconv,dil,T", [(1, 2, 3), (3, 3, 17), (7, 4, 113), (7, 2, 208)])
def test_integer_chain_cases_are_exact(fmt, nconv, dil, T):
    """the GPU's integer sweep relies on these operands never rounding: the reference asserts it"""
    U, Ws, bs, ss, hs = R.integer_chain_case(2, T, nconv, fmt, seed=T + nconv)
    ys = R.res2net_chain_ref(U, Ws, bs, ss, hs, nconv, T, dil, fmt, exact=True)
    assert len(ys) == nconv and all(float(y.abs().max()) < 256 for y in ys)
    assert any(float(y.abs().max()) > 0 for y in ys)


def test_bounds_catch_a_single_pass_variance():
    """the pooling bound is tight enough to fail the single pass about h[t = 0] that the fused ASP kernels used (emulated in fp32):
    frame 0 at 50 sigma, attention peaked away from it"""
    rng = np.random.default_rng(0)
    T = 201
    h = R.store(torch.from_numpy(rng.standard_normal(T)), 0)
    h[0] = 50.0
    lg = torch.from_numpy(rng.standard_normal(T) * 0.5)
    lg[100:110] += 6
    want, err = R.asp_pool_ref(lg.float()[:, None], h[:, None], 1, T)
    e = np.exp((lg - lg.max()).numpy().astype(np.float32)).astype(np.float32)
    d = (h.numpy().astype(np.float32) - np.float32(h[0]))
    l = s1 = s2 = np.float32(0)
    for i in range(T):
        l = np.float32(l + e[i])
        s1 = np.float32(s1 + e[i] * d[i])
        s2 = np.float32(s2 + np.float32(e[i] * d[i]) * d[i])
    a = np.float32(s1 / l)
    sd1 = float(np.sqrt(max(np.float32(s2 / l) - a * a, 1e-12)))
    assert abs(sd1 - float(want[0, 1])) > 3 * float(err[0, 1])          # this fp32 emulation: 6 x the bound
