"""GPU checks of the PyanNet segmentation kernels (csrc/segmentation.hip) in bf16 (precision 0) and fp16 (precision 2).

Bounds: for every check, the reference model's own spread is measured first - the largest |difference| between the rounded model with fp32
accumulation and the same model with float64 accumulation, on the same inputs (tests/segmentation_ref.py) - and the GPU must lie within 3x that
spread of the fp32-accumulating model: the factor covers the kernels' different (fixed) summation order, as for the ResNet34 family.  Each
test prints its figures before it asserts."""
from __future__ import annotations

import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from segmentation_ref import SegRef, mixed_audio  # noqa: E402

PKG = "speaker-diarization-toolkit_amd"
seg = importlib.import_module(f"{PKG}.segmentation")
pytestmark = pytest.mark.gpu
FMT = {0: "bf16", 2: "fp16"}
FACTOR = 3.0
WEIGHT_KW = dict(lstm_gain=3.5, recurrent_gain=1.0, classifier_gain=20.0)


@pytest.fixture(scope="module")
def weights():
    return seg.synthetic_weights(0, **WEIGHT_KW)


@pytest.fixture(scope="module")
def models(engine, weights):
    return {p: seg.Segmentation(engine, weights, precision=p) for p in (0, 2)}


def refs(weights, prec):
    return SegRef(weights, FMT[prec], torch.float32), SegRef(weights, FMT[prec], torch.float64)


def maxdiff(a, b) -> float:
    return float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs().max())


def dev(pcm):
    return torch.from_numpy(np.ascontiguousarray(pcm)).cuda()


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("S", [991, 32000, 160000])
@pytest.mark.parametrize("B", [1, 7, 37])
def test_forward_within_bound(models, weights, prec, S, B):
    pcm = mixed_audio(B, S, seed=B * 7 + S % 1000)
    r32, r64 = refs(weights, prec)
    want = r32.forward(pcm)
    spread = maxdiff(want, r64.forward(pcm))
    got = models[prec].forward(dev(pcm))
    torch.cuda.synchronize()
    assert got.shape == (B, seg.num_frames(S), 7)
    err = maxdiff(got.cpu(), want)
    print(f"forward prec={prec} S={S} B={B}: spread {spread:.3e} bound {FACTOR * spread:.3e} gpu max|d| {err:.3e}")
    assert np.isfinite(err) and err <= FACTOR * spread


@pytest.mark.parametrize("prec", [0, 2])
def test_frontend_within_bound(models, weights, prec):
    for B, S in ((7, 32000), (3, 160000)):
        pcm = mixed_audio(B, S, seed=11 + B)
        r32, r64 = refs(weights, prec)
        want = r32.frontend(pcm)
        spread = maxdiff(want, r64.frontend(pcm))
        got = models[prec].frontend(dev(pcm))
        torch.cuda.synchronize()
        F = seg.num_frames(S)
        g = got.float().cpu().reshape(B, F, 64)
        assert torch.all(g[:, :, 60:] == 0)
        err = maxdiff(g[:, :, :60], want)
        print(f"frontend prec={prec} S={S} B={B}: spread {spread:.3e} bound {FACTOR * spread:.3e} gpu max|d| {err:.3e}")
        assert err <= FACTOR * spread


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("layer", [0, 1])
def test_bilstm_layer_within_bound(models, weights, prec, layer):
    B, S = 19, 32000
    pcm = mixed_audio(B, S, seed=5)
    r32, r64 = refs(weights, prec)
    x = r32.frontend(pcm)
    if layer == 1:
        x = r32.lstm_layer(0, x)
    want = r32.lstm_layer(layer, x)
    spread = maxdiff(want, r64.lstm_layer(layer, x.double()))
    F = x.shape[1]
    xin = torch.zeros(B * F, 64 if layer == 0 else 256, dtype=torch.float32)
    xin[:, :x.shape[2]] = x.reshape(B * F, -1).float()
    got = models[prec].bilstm_layer(layer, xin.cuda(), B, F)
    torch.cuda.synchronize()
    err = maxdiff(got.float().cpu().reshape(B, F, 256), want)
    print(f"bilstm layer {layer} prec={prec} B={B} F={F}: spread {spread:.3e} bound {FACTOR * spread:.3e} gpu max|d| {err:.3e}")
    assert err <= FACTOR * spread


@pytest.mark.parametrize("prec", [0, 2])
def test_powerset_argmax(models, weights, prec):
    """Frames whose float64-model top-two margin is at most 2x the bound are excluded (at most 3 % of them); every other frame's argmax
    equals the float64 model's.  The inputs are first checked to make the agreement non-trivial: >= 3 classes win >= 2 % of the frames."""
    pcm = mixed_audio(8, 160000, seed=1)
    r32, r64 = refs(weights, prec)
    want32, want64 = r32.forward(pcm), r64.forward(pcm)
    bound = FACTOR * maxdiff(want32, want64)
    lp = want64.reshape(-1, 7)
    top2 = lp.topk(2, dim=1).values
    excl = (top2[:, 0] - top2[:, 1]) <= 2 * bound
    shares = np.bincount(lp.argmax(1).numpy(), minlength=7) / lp.shape[0]
    print(f"powerset prec={prec}: bound {bound:.3e}, class shares {np.round(shares, 4).tolist()}, excluded {float(excl.double().mean()):.4f}")
    assert (shares >= 0.02).sum() >= 3
    assert float(excl.double().mean()) <= 0.03
    got = models[prec].forward(dev(pcm))
    ga = torch.argmax(got, dim=-1).cpu().reshape(-1)
    keep = ~excl
    mism = int((ga[keep] != lp.argmax(1)[keep]).sum())
    print(f"powerset prec={prec}: {mism} mismatching frames of {int(keep.sum())}")
    assert mism == 0
    assert torch.equal(seg.speaker_count(got).cpu().reshape(-1), torch.tensor([len(c) for c in seg.POWERSET])[ga])


@pytest.mark.parametrize("prec", [0, 2])
def test_starts_and_determinism(models, prec):
    rng = np.random.default_rng(3)
    rec = mixed_audio(1, 16000 * 23 + 777, seed=9)[0]
    st = np.array([0, 16000, 16000 * 13 + 5, len(rec) - 160000, len(rec) - 40000], np.int32)    # the last runs past the end: zero-filled
    rows = np.zeros((len(st), 160000), np.int16)
    for i, s in enumerate(st):
        piece = rec[s:s + 160000]
        rows[i, :len(piece)] = piece
    m = models[prec]
    a = m.forward(dev(rec), torch.from_numpy(st).cuda())
    b = m.forward(dev(rows))
    c = m.forward(dev(rows))
    torch.cuda.synchronize()
    assert torch.equal(a, b), "windows cut through starts differ from the same windows as rows"
    assert torch.equal(b, c), "two runs differ"
    assert rng is not None


def test_errors(engine, models):
    from importlib import import_module
    SdkError = import_module(f"{PKG}._lib").SdkError
    m = models[0]
    pcm = dev(np.zeros((2, 990), np.int16))
    with pytest.raises(SdkError, match="S=990"):
        m.forward(pcm)
    with pytest.raises(ValueError, match="precision 1"):
        seg.Segmentation(engine, m.weights, precision=1)
    lib = engine.lib
    d = seg.SegmentationDesc()
    C.memmove(C.byref(d), C.byref(m.desc), C.sizeof(d))
    d.precision = 1
    x = dev(np.zeros((1, 32000), np.int16))
    out = torch.empty((1, seg.num_frames(32000), 7), device="cuda")
    ws = torch.empty(lib.sdk_segmentation_workspace_bytes(C.byref(m.desc), 1, 32000), dtype=torch.uint8, device="cuda")
    from_ops = import_module(f"{PKG}.ops")
    rc = lib.sdk_segmentation_forward(engine.ctx, m.blob.data_ptr(), C.byref(d), x.data_ptr(), x.numel(), None, 32000, 1, 32000, ws.data_ptr(),
                                      ws.numel(), out.data_ptr(), from_ops._stream())
    assert rc != 0 and b"precision 1" in lib.sdk_last_error()
    rc = lib.sdk_segmentation_forward(engine.ctx, m.blob.data_ptr(), C.byref(m.desc), x.data_ptr(), x.numel(), None, 32000, 1, 32000, ws.data_ptr(),
                                      ws.numel() - 256, out.data_ptr(), from_ops._stream())
    assert rc != 0 and b"workspace" in lib.sdk_last_error()
    out.fill_(7.0)
    rc = lib.sdk_segmentation_forward(engine.ctx, m.blob.data_ptr(), C.byref(m.desc), x.data_ptr(), x.numel(), None, 32000, 0, 32000, None, 0,
                                      out.data_ptr(), from_ops._stream())
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.all(out == 7.0)), "B = 0 must be a no-op"
    rc = lib.sdk_bilstm_layer(engine.ctx, m.blob.data_ptr(), C.byref(m.desc), 4, x.data_ptr(), 256, 1, 10, ws.data_ptr(), ws.numel(), out.data_ptr(),
                              from_ops._stream())
    assert rc != 0 and b"layer=4" in lib.sdk_last_error()


def test_backend_speech_ranges(tmp_path, monkeypatch):
    monkeypatch.setenv("SDK_MODEL", "resnet34")
    monkeypatch.delenv("SDK_NO_TORCH", raising=False)
    monkeypatch.delenv("SDK_SEGMENTATION_WEIGHTS", raising=False)
    backend = importlib.import_module(f"{PKG}.backend")
    be = backend.Backend()
    n = 16000 * 14 + 1234
    samples = mixed_audio(1, n, seed=21)[0]
    speech, overlap = be.speech_ranges(samples, step_s=1.0)
    # the rule applied to the GPU's own per-chunk counts
    m = be.segmentation()
    st = seg.chunk_starts(n, 1.0)
    logp = m.forward(dev(samples), torch.from_numpy(st.astype(np.int32)).cuda())
    counts = seg.speaker_count(logp).cpu().numpy()
    assert (speech, overlap) == seg.aggregate_counts(counts, st, n)
    print(f"speech_ranges: {len(speech)} speech ranges, {len(overlap)} overlap ranges")
    if speech:
        labels, wins, range_labels = be.cluster_ranges(samples, speech, threshold=0.5, min_cluster_size=1)
        assert len(range_labels) == len(speech)
    short = mixed_audio(1, 5000, seed=2)[0]
    sp, ov = be.speech_ranges(short)
    assert all(0 <= a < b for a, b in sp + ov)
