"""CPU checks of the masked attentive statistics pooling's references (tests/asp_masked_ref.py) against the unmasked ones, of the C ABI's
new exports, of the SDK_DIARIZE_MODEL option and of ecapa_diar.EcapaEmbedder's surface.  No GPU."""
import re

import numpy as np
import pytest
import torch

import asp_masked_ref as MR
import sweeps_ref as R
from conftest import ROOT, sub
from oracle import ecapa as oecapa

L = sub("_lib")
W = sub("weights")
SMALL = W.EcapaConfig(channels=256, mfa_channels=768, res2net_scale=2, se_channels=64, attn_channels=128)


def _data(B, T, C, seed):
    g = torch.Generator().manual_seed(seed)
    h = R.store(torch.randn(B * T, C, generator=g) * 2 + 1, 0)
    lg = (torch.rand(B * T, C, generator=g) * 40 - 20).float().double()
    return h, lg, g


def test_all_ones_weights_are_the_unmasked_references():
    B, T, C = 2, 37, 16
    h, lg, _ = _data(B, T, C, 1)
    want, bound = MR.asp_stats_masked_ref(h, torch.ones(B, 1, T), B, T)
    ref, _ = R.asp_stats_ref(h, B, T)
    assert float((want - ref).abs().max()) <= 1e-12 and (bound > 0).all()
    want, bound = MR.asp_pool_masked_ref(lg, h, torch.ones(B, T), B, T)
    ref, _ = R.asp_pool_ref(lg, h, B, T)
    assert float((want - ref).abs().max()) <= 1e-12 and (bound > 0).all()


def test_binary_mask_is_the_unmasked_reference_on_the_gathered_frames():
    B, T, C = 1, 41, 8
    h, lg, g = _data(B, T, C, 2)
    m = torch.rand(T, generator=g) < 0.4
    m[3] = True
    n = int(m.sum())
    want, _ = MR.asp_stats_masked_ref(h, m.double().reshape(1, 1, T), B, T)
    ref, _ = R.asp_stats_ref(h[m], 1, n)
    assert float((want - ref).abs().max()) <= 1e-12
    lg2 = lg.clone()
    lg2[~m] = float("nan")                                              # masked-out logits enter nothing
    want, bound = MR.asp_pool_masked_ref(lg2, h, m.double().reshape(1, T), B, T)
    ref, _ = R.asp_pool_ref(lg[m], h[m], 1, n)
    assert float((want - ref).abs().max()) <= 1e-12 and torch.isfinite(bound).all()
    # fractional weights: the weighted definitions, restated with numpy
    w = torch.rand(1, 2, T, generator=g).double()
    w[0, 1] = 0
    want, bound = MR.asp_stats_masked_ref(h, w, B, T)
    mu = np.average(h.numpy(), axis=0, weights=w[0, 0].numpy())
    assert np.abs(want[0, :C].numpy() - mu).max() <= 1e-12
    assert not want[1].any() and not bound[1].any(), "a row without weight is zeros"


def test_masked_oracle_equals_the_oracle_with_all_ones_weights():
    wts = W.synthetic_weights(3, SMALL)
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(2, 40, 80, generator=g)
    for acc in (torch.float64, torch.float32):
        a = oecapa.EcapaOracle(wts, "bf16", acc, n_dilations=SMALL.dilations, scale=SMALL.res2net_scale)
        b = MR.MaskedEcapaOracle(wts, "bf16", acc, n_dilations=SMALL.dilations, scale=SMALL.res2net_scale)
        pa, ia = a.forward_pooled(feats)
        pb, ib = b.forward_pooled(feats)
        assert torch.equal(ia["mfa"], ib["mfa"]), "the trunk is the parent's"
        # both oracles store pooled as fp32; the masked one's float64 values BEFORE that store are within 1e-12 of the parent's, so the
        # parent's fp32 value is the rounding of a number within 1e-12 of p64: half an fp32 ulp (2^-24 |p64|) + 1e-12, and equal to
        # p64's own rounding except on a rounding boundary.  (acc = float32 moves the GEMMs only, and both run the same ones: same bound)
        p64 = b.pool_masked(ib["mfa"], torch.ones(2, 1, 40), as64=True)[:, 0]
        assert ((pa.double() - p64).abs() <= 2.0 ** -24 * p64.abs() + 1e-12).all(), acc
        assert float((pa == p64.float()).double().mean()) >= 0.999 and torch.equal(pb, p64.float())
        assert float((a.embed(feats).double() - b.embed(feats).double()).abs().max()) <= 1e-5
    w = torch.rand(2, 3, 40, generator=g)
    w[1, 2] = 0
    e = b.embed_masked(feats, w)
    e2 = b.embed_masked(feats, torch.cat([w[:, :1] * 0 + 1, w[:, 1:]], 1))
    assert e.shape == (2, 3, SMALL.embed_dim) and not e[1, 2].any() and e[0, 2].any()
    assert torch.equal(e[:, 1], e2[:, 1]), "a row depends on its own weights only"


def test_new_symbols_are_exported_and_the_abi_version_stays():
    names = ("sdk_ecapa_masked_workspace_bytes", "sdk_ecapa_forward_masked", "sdk_asp_stats_masked_fmt", "sdk_asp_pool_masked_fmt")
    header = (ROOT / "include" / "sdk_hip.h").read_text()
    for n in names:
        assert n in L.SIGNATURES and re.search(rf"\b{n}\(", header), n
    assert re.search(r"#define SDK_ABI_VERSION 4\b", header) and L.ABI_VERSION == 4
    if L.LIB_PATH.exists():
        lib = L.load_library()
        assert lib.sdk_abi_version() == 4
        for n in names:
            assert getattr(lib, n) is not None
        d = L.EcapaDesc()
        assert lib.sdk_ecapa_masked_workspace_bytes(None, 1, 100, 3) == 0
        d.precision = 1
        assert lib.sdk_ecapa_masked_workspace_bytes(d, 1, 100, 3) == 0


def test_sdk_diarize_model_is_parsed(monkeypatch, capsys):
    B = sub("backend")
    for k in ("SDK_MODEL", "SDK_DIARIZE_MODEL", "SDK_PRECISION", "SDK_NO_TORCH", "SDK_COHORT", "SDK_COHORT_THRESHOLD"):
        monkeypatch.delenv(k, raising=False)
    assert B.Backend().diarize_model == "resnet34"
    monkeypatch.setenv("SDK_DIARIZE_MODEL", "ECAPA ")
    assert B.Backend().diarize_model == "ecapa"
    monkeypatch.setenv("SDK_PRECISION", "2")
    assert B.Backend().diarize_model == "ecapa"
    monkeypatch.setenv("SDK_PRECISION", "1")
    with pytest.raises(ValueError, match=r"SDK_DIARIZE_MODEL=ecapa requires SDK_PRECISION 0 \(bf16\) or 2 \(fp16\)"):
        B.Backend()
    monkeypatch.delenv("SDK_PRECISION")
    monkeypatch.setenv("SDK_MODEL", "resnet34")
    with pytest.raises(ValueError, match=r"SDK_DIARIZE_MODEL=ecapa .* requires SDK_MODEL=ecapa, got SDK_MODEL='resnet34'"):
        B.Backend()
    monkeypatch.setenv("SDK_MODEL", "ecapa")
    monkeypatch.setenv("SDK_DIARIZE_MODEL", "wavlm")
    with pytest.raises(ValueError, match=r"SDK_DIARIZE_MODEL='wavlm': expected 'resnet34' \(default\) or 'ecapa'"):
        B.Backend()
    # link_speakers: the refusal names both ways
    monkeypatch.delenv("SDK_DIARIZE_MODEL")
    with pytest.raises(ValueError, match=r"link_speakers: candidates.*SDK_MODEL=resnet34, or with SDK_MODEL=ecapa and SDK_DIARIZE_MODEL=ecapa"):
        B.Backend().link_speakers([], candidates=[])


def test_ecapa_embedder_has_the_four_members():
    ED = sub("ecapa_diar")

    class Eng:
        cfg = W.DEFAULT_CONFIG
        precision = 0
        bias_correction = False
        calls = []

        def set_precision(self, p):
            self.precision = p

        def ecapa_forward_masked(self, *a):
            self.calls.append((self.precision,) + a)
            return "emb"

    eng = Eng()
    e = ED.EcapaEmbedder(eng, precision=2)
    assert e.cfg.embed_dim == 192 and e.precision == 2 and e.last_map_frames(1001) == 1001
    assert e.forward_masked("f", 2, 1001, "w", "v") == "emb" and eng.calls == [(2, "f", 2, 1001, "w", "v")]
    assert ED.EcapaEmbedder(Eng()).precision == 0
    with pytest.raises(ValueError, match=r"precision 1 is not served.*modes 0 \(bf16\) and 2 \(fp16\)"):
        ED.EcapaEmbedder(eng, precision=1)
    dz = sub("diarize")
    d = dz.Diarizer(eng, None, e)
    assert d.embedder is e and d.resnet is e
    with pytest.raises(AttributeError):
        d.embedder = None
