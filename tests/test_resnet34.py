"""The ResNet34 family (resnet.py; the WeSpeaker ResNet34 PyAnnote 3.1 embeds with).  CPU: the layer-boundary model against an independently
composed torch.nn ResNet34, the hand counts, the packer (BN folding, tap-major K, the projection shortcut's columns, slots), the C structs, the
Backend's metadata and refusals.  GPU: sdk_resnet_conv2d bit-exact on small-integer operands for every layer shape, sdk_resnet_forward against the
layer-boundary model (bf16 and fp16), batch invariance and determinism, PCM -> fbank -> ResNet34 -> L2 -> k4, and the Backend round trip."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import sub
import resnet_ref as RR

RN = sub("resnet")
LIB = sub("_lib")
WP = sub("weights_pack")

LAYER_SHAPES = [(1, 32, 1), (32, 32, 1), (32, 64, 2), (64, 64, 1), (64, 128, 2), (128, 256, 2), (256, 256, 1)]


def _cos(a, b):
    a, b = a.double(), b.double()
    return (a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1))


# ------------------------------------------------------------------------------------------------------------------------------- CPU
def test_layer_boundary_model_without_rounding_equals_torch_nn():
    w = RN.synthetic_weights(3)
    feats = torch.randn(2, 37, 80, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 3
    with torch.no_grad():
        ref = RR.torch_resnet34(w)(feats)
        got = RR.layer_boundary_embed(w, feats, bits=None)
    assert got.shape == (2, 192)
    assert float((got - ref).abs().max()) < 1e-5, float((got - ref).abs().max())


def test_param_count_and_macs_are_the_hand_counts():
    cfg = RN.DEFAULT_RESNET
    bn = 4
    params = 32 * 9 + bn * 32                                                             # stem
    params += 3 * (2 * 9 * 32 * 32 + 2 * bn * 32)                                         # layer1
    for cin, c, nb in ((32, 64, 4), (64, 128, 6), (128, 256, 3)):
        params += 9 * c * cin + 9 * c * c + 2 * bn * c + c * cin + bn * c                 # first block + projection shortcut
        params += (nb - 1) * (2 * 9 * c * c + 2 * bn * c)
    params += 192 * 5120 + 192                                                            # seg_1
    assert cfg.param_count() == params == 6315104
    assert cfg.map_sizes(201) == [(80, 201), (80, 201), (40, 101), (20, 51), (10, 26)]
    l1 = 6 * 80 * 201 * 32 * 9 * 32
    l2 = 40 * 101 * 64 * (9 * 32 + 7 * 9 * 64 + 32)
    l3 = 20 * 51 * 128 * (9 * 64 + 11 * 9 * 128 + 64)
    l4 = 10 * 26 * 256 * (9 * 128 + 5 * 9 * 256 + 128)
    assert [round(2 * m / 1e9, 2) for m in (l1, l2, l3, l4)] == [1.78, 2.25, 3.48, 1.7]
    assert cfg.macs_per_segment(201) == 80 * 201 * 32 * 9 + l1 + l2 + l3 + l4 + 5120 * 192
    assert abs(2 * cfg.macs_per_segment(201) / 1e9 - 9.22) < 0.01


def _slot(blob, d, i, shape, dtype):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return blob[d.off[i]:d.off[i] + n].view(dtype).reshape(shape)


def test_packer_folds_bn_orders_taps_and_appends_the_shortcut():
    w = RN.synthetic_weights(1)
    blob, d = RN.pack_weights(w)
    assert list(d.blocks) == [3, 4, 6, 3] and list(d.width) == [32, 64, 128, 256] and d.n_feats == 80 and d.embed_dim == 192 and d.precision == 0

    def fold(bn):
        s = w[f"{bn}.weight"].astype(np.float64) / np.sqrt(w[f"{bn}.running_var"].astype(np.float64) + 1e-5)
        return s, w[f"{bn}.bias"] - w[f"{bn}.running_mean"] * s

    s, sh = fold("bn1")                                                                   # stem: [32][9], k = 3 dy + dx
    stem = _slot(blob, d, 0, (32, 9), np.uint16)
    assert np.array_equal(stem, WP.f32_to_bf16_bits((w["conv1.weight"][:, 0].astype(np.float64) * s[:, None, None]).astype(np.float32).reshape(32, 9)))
    assert np.allclose(_slot(blob, d, 1, (32,), np.float32), sh, rtol=0, atol=1e-6)
    # layer2.0.conv2 = conv index 1 + 2 * 3 + 1 = 8: K = 9 * 64 tap-major, then the shortcut's 32 columns; bias = both shifts
    s2, sh2 = fold("layer2.0.bn2")
    ss, shs = fold("layer2.0.shortcut.1")
    k = _slot(blob, d, 16, (64, 9 * 64 + 32), np.uint16)
    w2 = w["layer2.0.conv2.weight"].astype(np.float64) * s2[:, None, None, None]
    for co, c, dy, dx in ((0, 0, 0, 0), (5, 17, 1, 2), (63, 63, 2, 1), (31, 40, 2, 0)):
        assert k[co, (3 * dy + dx) * 64 + c] == WP.f32_to_bf16_bits(np.float32(w2[co, c, dy, dx]).reshape(1))[0]
    assert np.array_equal(k[:, :576], WP.f32_to_bf16_bits(np.transpose(w2, (0, 2, 3, 1)).reshape(64, 576).astype(np.float32)))
    assert np.array_equal(k[:, 576:], WP.f32_to_bf16_bits((w["layer2.0.shortcut.0.weight"][:, :, 0, 0] * ss[:, None]).astype(np.float32)))
    assert np.allclose(_slot(blob, d, 17, (64,), np.float32), sh2 + shs, rtol=0, atol=1e-6)
    # an identity block keeps K = 9 C; seg_1 transposed
    assert RN.folded_convs(w)[3][1].shape == (32, 288) and RN.folded_convs(w)[9][1].shape == (64, 576)
    assert np.array_equal(_slot(blob, d, 66, (5120, 192), np.float32), w["seg_1.weight"].T)
    # slots: 33 convs, every slot 256-byte aligned, no two overlapping
    offs = sorted(int(o) for o in list(d.off)[:66] + [d.off[66], d.off[67]])
    assert all(o % 256 == 0 for o in offs) and len(set(offs)) == 68 and all(o == -1 for o in list(d.off)[68:])
    # fp16 mode: the same layout with fp16 bits
    b2, d2 = RN.pack_weights(w, precision=2)
    assert d2.precision == 2 and list(d2.off) == list(d.off)
    assert np.array_equal(_slot(b2, d2, 16, (64, 608), np.uint16)[:, :576], WP.f32_to_f16_bits(np.transpose(w2, (0, 2, 3, 1)).reshape(64, 576).astype(np.float32)))


def test_packer_refuses_bad_shapes_and_the_precise_mode():
    w = RN.synthetic_weights(0)
    bad = dict(w)
    bad["layer3.2.conv1.weight"] = bad["layer3.2.conv1.weight"][:, :-1]
    with pytest.raises(ValueError, match=r"layer3\.2\.conv1\.weight"):
        RN.pack_weights(bad)
    with pytest.raises(ValueError, match="seg_1.bias"):
        RN.pack_weights({k: v for k, v in w.items() if k != "seg_1.bias"})
    with pytest.raises(ValueError, match="SDK_PRECISION"):
        RN.pack_weights(w, precision=1)


def test_struct_sizes():
    assert C.sizeof(RN.ResNetDesc) == 4 * 4 + 8 * 4 + 72 * 8 == 624
    assert C.sizeof(LIB.ResNetConvArgs) == 7 * 8 + 12 * 4 == 104
    assert LIB.KERNEL_FAMILIES[-3:] == ["resnet_conv", "resnet_stem", "resnet_pool"]


def test_backend_resnet34_metadata(monkeypatch, tmp_path):
    B = sub("backend")
    monkeypatch.setenv("SDK_MODEL", "resnet34")
    monkeypatch.delenv("SDK_RESNET_WEIGHTS", raising=False)
    be = B.Backend()
    assert be.model == "resnet34" and be.embedding_dim == 192 and be.name == "mi355x"
    mv = be.model_version
    assert mv == f"mi355x-resnet34-{sub('weights').weights_digest(RN.synthetic_weights(0))}" and len(mv.split("-")[-1]) == 12
    assert be.check_embedding_compatibility({"model_version": mv})["compatible"] is True
    assert be.numerics()["bias_correction"] is False
    w = RN.synthetic_weights(4)
    np.savez(tmp_path / "rn.npz", **w)
    monkeypatch.setenv("SDK_RESNET_WEIGHTS", str(tmp_path / "rn.npz"))
    assert B.Backend().model_version == f"mi355x-resnet34-{sub('weights').weights_digest(w)}"
    bad = dict(w); bad["seg_1.weight"] = bad["seg_1.weight"][:, :-1]
    np.savez(tmp_path / "bad.npz", **bad)
    monkeypatch.setenv("SDK_RESNET_WEIGHTS", str(tmp_path / "bad.npz"))
    with pytest.raises(ValueError, match="seg_1.weight"):
        B.Backend().model_version
    monkeypatch.setenv("SDK_MODEL", "resnet")
    with pytest.raises(ValueError, match="SDK_MODEL"):
        B.Backend()


def test_backend_resnet34_refuses_the_torch_free_path(monkeypatch):
    monkeypatch.setenv("SDK_MODEL", "resnet34")
    monkeypatch.setenv("SDK_NO_TORCH", "1")
    be = sub("backend").Backend()
    with pytest.raises(ValueError, match=r"SDK_NO_TORCH=1 with SDK_MODEL=resnet34"):
        be.engine()


def test_store_refuses_vectors_of_another_family(tmp_path):
    """The exact model_version match keeps the families apart: an ECAPA-TDNN vector is skipped, with its reason, by a ResNet34 load."""
    store = sub("store")
    rng = np.random.default_rng(0)
    v = rng.standard_normal(192).astype(np.float32)
    ext_e = store.save_vector(v / np.linalg.norm(v), root=tmp_path)
    v = rng.standard_normal(192).astype(np.float32)
    ext_r = store.save_vector(v / np.linalg.norm(v), root=tmp_path)
    mv_r, mv_e = "mi355x-resnet34-0123456789ab", "mi355x-ecapa1024-0123456789ab"
    cands = [{"id": "a", "names": {"default": "a"}, "embeddings": {"mi355x": [{"id": "e1", "external_id": ext_e, "model_version": mv_e}]}},
             {"id": "b", "names": {"default": "b"}, "embeddings": {"mi355x": [{"id": "e2", "external_id": ext_r, "model_version": mv_r}]}}]
    batch = store.load_profile_batch(cands, "mi355x", model_prefix="mi355x-", root=tmp_path, link=False, model_version=mv_r, use_pack=False)
    assert batch.speaker_ids == ["b"] and any("enrolled under mi355x-ecapa1024" in s for s in batch.skipped)


# ------------------------------------------------------------------------------------------------------------------------------- GPU
def _conv(engine, x, wk, bias, B, F, T, Cin, Cout, stride, f16=False, sc=None, Csc=0, Fsc=0, Tsc=0, sc_stride=0, res=None, ldx=0, relu=True):
    Fo, To = (F - 1) // stride + 1, (T - 1) // stride + 1
    dt = torch.float16 if f16 else torch.bfloat16
    y = torch.full((B, Fo, To, Cout), 777.0, dtype=dt, device="cuda")
    a = LIB.ResNetConvArgs()
    a.x, a.W, a.bias, a.y, a.ldx = x.data_ptr(), wk.data_ptr(), bias.data_ptr(), y.data_ptr(), ldx
    a.sc = sc.data_ptr() if sc is not None else None
    a.res = res.data_ptr() if res is not None else None
    a.B, a.F, a.T, a.Cin, a.Cout, a.stride = B, F, T, Cin, Cout, stride
    a.Csc, a.Fsc, a.Tsc, a.stride_sc = Csc, Fsc, Tsc, sc_stride
    a.flags = (LIB.GEMM_RELU if relu else 0) | (LIB.GEMM_F16 if f16 else 0)
    LIB.check(engine.lib.sdk_resnet_conv2d(engine.ctx, C.byref(a), None), "sdk_resnet_conv2d")
    torch.cuda.synchronize()
    return y.cpu()


def _ints(g, shape, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


@pytest.mark.gpu
@pytest.mark.parametrize("T", [9, 37, 51, 201])
@pytest.mark.parametrize("Cin,Cout,stride", LAYER_SHAPES)
def test_conv2d_integer_exact(engine, Cin, Cout, stride, T):
    """Small-integer operands: the fp32 accumulation is exact, so the GPU must equal the float64 conv rounded once to bf16, bit for bit.  Every
    layer shape; the same-width stride-1 shapes with their identity residual; B = 3 segments; the stem reads the fbank matrix with its padding
    columns set to a sentinel that would show if they were read."""
    g = torch.Generator().manual_seed(Cin * 1000 + T)
    B = 3
    bias = _ints(g, (Cout,), -4, 4)
    if Cin == 1:
        F, ldf = 80, 88
        img = _ints(g, (B, T, F))
        feats = torch.full((B * T, ldf), 1000.0, dtype=torch.bfloat16)
        feats[:, :F] = img.reshape(B * T, F).to(torch.bfloat16)
        wk = _ints(g, (Cout, 9))
        got = _conv(engine, feats.cuda(), wk.to(torch.bfloat16).cuda(), bias.float().cuda(), B, F, T, 1, Cout, 1, ldx=ldf)
        want = RR.conv_ref(img.transpose(1, 2).unsqueeze(-1), wk, bias, 1)
    else:
        F = 6 if stride == 1 else 7
        x = _ints(g, (B, F, T, Cin))
        wk = _ints(g, (Cout, 9 * Cin))
        Fo, To = (F - 1) // stride + 1, (T - 1) // stride + 1
        res = _ints(g, (B, Fo, To, Cout), -8, 8) if (Cin == Cout and stride == 1) else None
        got = _conv(engine, x.to(torch.bfloat16).cuda(), wk.to(torch.bfloat16).cuda(), bias.float().cuda(), B, F, T, Cin, Cout, stride,
                    res=res.to(torch.bfloat16).cuda() if res is not None else None)
        want = RR.conv_ref(x, wk, bias, stride, res=res)
    assert got.shape == want.shape
    assert torch.equal(got, want.to(torch.bfloat16)), float((got.double() - want.to(torch.bfloat16).double()).abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("T", [9, 37, 51, 201])
@pytest.mark.parametrize("Cin,C", [(32, 64), (64, 128), (128, 256)])
def test_conv2d_fused_projection_shortcut_integer_exact(engine, Cin, C, T, f16):
    """A downsampling block's conv2 with its 1x1 stride-2 projection shortcut as extra K columns (K = 9 C + Cin), bf16 and fp16 storage."""
    g = torch.Generator().manual_seed(C * 1000 + T)
    B, Fin = 3, 9
    Tin = T
    F, Tm = (Fin - 1) // 2 + 1, (Tin - 1) // 2 + 1
    dt = torch.float16 if f16 else torch.bfloat16
    xin = _ints(g, (B, Fin, Tin, Cin))
    h = _ints(g, (B, F, Tm, C))
    wk = _ints(g, (C, 9 * C))
    wsc = _ints(g, (C, Cin))
    bias = _ints(g, (C,), -4, 4)
    got = _conv(engine, h.to(dt).cuda(), torch.cat([wk, wsc], 1).to(dt).cuda(), bias.float().cuda(), B, F, Tm, C, C, 1, f16=f16,
                sc=xin.to(dt).cuda(), Csc=Cin, Fsc=Fin, Tsc=Tin, sc_stride=2)
    want = RR.conv_ref(h, wk, bias, 1, sc=xin, wsc=wsc, sc_stride=2)
    assert torch.equal(got, want.to(dt)), float((got.double() - want.to(dt).double()).abs().max())


def _feats(B, T, seed, dt=torch.bfloat16, ldf=None):
    """Random features in the storage format (as the front end writes them) + the device matrix [B*T, ldf] with sentinel padding columns."""
    ldf = ldf or WP.N_MELS_PADDED
    x = (torch.randn(B, T, 80, generator=torch.Generator().manual_seed(seed)) * 3.0).to(dt)
    f = torch.zeros(B * T, ldf, dtype=dt)
    f[:, :80] = x.reshape(-1, 80)
    f[:, 80:] = 5.0                                                          # must never be read as data
    return x.double(), f.cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", [(4, 201), (3, 51), (2, 101), (1, 9)])
def test_resnet_forward_matches_the_layer_boundary_model(engine, B, T):
    """The full forward against the layer-boundary model: bf16, fp32 (cos > 0.999), and precision 2 against the 11-bit model.
    Bounds: the x-vector test's (cos > 1 - 2e-5, 2e-3 max|want|) do not fit a 33-conv network.  The model's OWN spread - the same rounding sites
    evaluated with fp32 instead of float64 accumulation, on the CPU, at these inputs - reaches 1 - cos = 3.2e-5 and 9.0e-3 max|want| in bf16
    (at T = 9, where the last map has 2 frames) and 5.8e-7 / 1.2e-3 in fp16: an accumulation-order difference flips a last bit at one of 33
    rounding sites and the flip travels.  The bounds below are about 3x those spreads."""
    w = RN.synthetic_weights(0)
    rn = RN.ResNet34(engine, w)
    x, f = _feats(B, T, seed=T)
    emb = rn.forward(f, B, T).cpu()
    torch.cuda.synchronize()
    want = RR.layer_boundary_embed(w, x, bits=8)
    assert (_cos(emb, want) > 1 - 1e-4).all(), _cos(emb, want)
    assert torch.allclose(emb.double(), want, rtol=0, atol=2.5e-2 * float(want.abs().max())), float((emb - want).abs().max())
    assert (_cos(emb, RR.layer_boundary_embed(w, x, bits=None)) > 0.999).all()
    rn2 = RN.ResNet34(engine, w, precision=2)
    x2, f2 = _feats(B, T, seed=T, dt=torch.float16)
    e2 = rn2.forward(f2, B, T).cpu()
    torch.cuda.synchronize()
    want2 = RR.layer_boundary_embed(w, x2, bits=11)
    print(f"\nResNet34 B={B} T={T}: 1 - cos bf16 {float((1 - _cos(emb, want)).max()):.2e}, fp16 {float((1 - _cos(e2, want2)).max()):.2e}; "
          f"max |d| / max |want| bf16 {float((emb - want).abs().max() / want.abs().max()):.2e}, fp16 {float((e2 - want2).abs().max() / want2.abs().max()):.2e}")
    assert (_cos(e2, want2) > 1 - 2e-6).all(), _cos(e2, want2)
    assert torch.allclose(e2.double(), want2, rtol=0, atol=4e-3 * float(want2.abs().max())), float((e2 - want2).abs().max())


@pytest.mark.gpu
def test_resnet_batch_invariance_and_determinism(engine):
    rn = RN.ResNet34(engine, RN.synthetic_weights(0))
    T, ldf = 201, WP.N_MELS_PADDED
    _, f = _feats(7, T, seed=11)
    e7 = rn.forward(f, 7, T).clone()
    again = rn.forward(f, 7, T).clone()
    singles = [rn.forward(f[i * T:(i + 1) * T], 1, T).clone() for i in range(7)]
    torch.cuda.synchronize()
    assert torch.equal(e7, again)
    for i, e in enumerate(singles):
        assert torch.equal(e[0], e7[i]), i
    assert f.stride(0) == ldf


@pytest.mark.gpu
def test_resnet_pcm_to_assignment_and_precise_mode_refusal(engine):
    """PCM -> fbank -> ResNet34 -> L2 -> cosine argmax on the shared 192-d k3 / k4; the precise mode is refused in Python and in C."""
    import importlib, sys
    from conftest import ROOT
    from oracle import scoring as oscoring
    sys.path.insert(0, str(ROOT))
    bench = importlib.import_module("bench")
    rn = RN.ResNet34(engine, seed=2)
    pcm = torch.from_numpy(bench.synth_pcm(40, seed=5)).cuda()
    E, Eb, re = rn.embed_pcm(pcm)
    assert E.shape == (40, 192) and float((E.double().norm(dim=1) - 1).abs().max()) < 1e-6
    P = bench.unit_rows(30, 192, seed=6)
    Pn, Pb, rp = engine.l2norm(torch.from_numpy(P).cuda())
    idx, sc = engine.affinity_topk(E, Eb, re, Pn, Pb, rp.max().reshape(1), k=1)
    torch.cuda.synchronize()
    oidx, osc = oscoring.affinity_topk(E.cpu().numpy(), Pn.cpu().numpy(), 1)
    assert np.array_equal(idx.cpu().numpy(), oidx) and np.abs(sc.cpu().numpy() - osc).max() <= 1e-5
    with pytest.raises(ValueError, match="SDK_PRECISION"):
        RN.ResNet34(engine, seed=2, precision=1)
    d = RN.ResNetDesc.from_buffer_copy(rn.desc)
    d.precision = 1
    ws = torch.empty(engine.lib.sdk_resnet_workspace_bytes(C.byref(d), 2, 201), dtype=torch.uint8, device="cuda")
    feats = engine.fbank(pcm[:2].contiguous())
    out = torch.empty(2, 192, device="cuda")
    rc = engine.lib.sdk_resnet_forward(engine.ctx, rn.blob.data_ptr(), C.byref(d), feats.data_ptr(), feats.stride(0), 2, 201, ws.data_ptr(),
                                       ws.numel(), out.data_ptr(), None)
    assert rc != 0 and b"precise mode" in engine.lib.sdk_last_error()


@pytest.mark.gpu
def test_backend_resnet34_enroll_identify_verify_roundtrip(tmp_path, monkeypatch):
    """The ResNet34 family through the drop-in boundary: stored vectors and window embeddings against the layer-boundary model on the same
    windows, identify / verify by the enrolled profiles; a vector enrolled under the ECAPA-TDNN is refused by the ResNet34 configuration."""
    from oracle import fbank as ofbank
    from oracle import ecapa as oecapa
    from test_gpu_backend_e2e import _voice
    wav = sub("wav")
    monkeypatch.setenv("SPEAKERS_EMBEDDINGS_DIR", str(tmp_path / "store"))
    monkeypatch.setenv("SDK_MODEL", "resnet34")
    monkeypatch.delenv("SDK_RESNET_WEIGHTS", raising=False)
    be = sub("backend").Backend()
    w = RN.synthetic_weights(0)

    def model_embed(pcm):
        x = RR.round_bits(torch.from_numpy(ofbank.fbank(pcm)).double(), 8)
        return oecapa.l2_normalise(RR.layer_boundary_embed(w, x, bits=8).numpy())

    profiles = []
    for i, (sid, f0) in enumerate({"alice": 140.0, "bob": 95.0}.items()):
        path = tmp_path / f"enroll_{sid}.wav"
        wav.write_wav_s16(path, _voice(10 + i, 6.0, f0))
        rec = be.enroll_speaker(path, [(0.5, 5.5)])
        assert rec["model_version"] == be.model_version and rec["model_version"].startswith("mi355x-resnet34-") and rec["embedding_dim"] == 192
        profiles.append({"id": sid, "names": {"default": sid}, "embeddings": {"mi355x": [
            {"id": f"emb-{sid}", "external_id": rec["external_id"], "model_version": rec["model_version"], "trust_level": "high"}]}})
        pcm, _ = wav.cut_windows(wav.read_wav_s16(path), [(0.5, 5.5)])
        e = model_embed(pcm).astype(np.float64).mean(0)
        assert float(np.load(rec["file"]) @ (e / np.linalg.norm(e))) > 1 - 1e-4, "stored enrollment vector vs the layer-boundary model"
    tpath = tmp_path / "meeting.wav"
    wav.write_wav_s16(tpath, np.concatenate([_voice(40, 4.0, 95.0), _voice(41, 4.0, 140.0)]))
    rows = be.identify_speaker(tpath, profiles, threshold=-1.0)
    assert {r["speaker_id"] for r in rows} <= {"alice", "bob"} and rows and all(r["confidence"] == r["similarity"] for r in rows)
    pcm, _ = wav.cut_windows(wav.read_wav_s16(tpath), None)
    E, Eb, re = be.embed_windows(pcm)
    assert ((E.cpu().numpy().astype(np.float64) * model_embed(pcm)).sum(1) > 1 - 1e-4).all()
    v = be.verify_speaker(tmp_path / "enroll_alice.wav", profiles[0], threshold=-1.0)
    assert v["match"] is True and v["embedding_id"] == "emb-alice" and v["similarity"] > 0.5, v
    # a vector enrolled under the ECAPA-TDNN: same backend name, other model_version -> refused, loudly
    monkeypatch.setenv("SDK_MODEL", "ecapa")
    ecapa_be = sub("backend").Backend()
    rec = ecapa_be.enroll_speaker(tmp_path / "enroll_alice.wav", [(0.5, 5.5)])
    assert rec["model_version"].startswith("mi355x-ecapa1024-")
    carol = {"id": "carol", "names": {"default": "carol"}, "embeddings": {"mi355x": [
        {"id": "emb-carol", "external_id": rec["external_id"], "model_version": rec["model_version"], "trust_level": "high"}]}}
    with pytest.raises(ValueError, match="enrolled under other weights"):
        be.identify_speaker(tpath, [carol])
