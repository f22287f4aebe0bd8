"""GPU checks of the many-recordings diarization (Diarizer.run_many, Backend.diarize_many): the grouped kernels of csrc/diarize.hip bit for
bit against the single-recording references applied recording by recording, the front end on a packed buffer against every recording alone,
and the whole pipeline against the CPU reference pipeline and against Diarizer.run.  Each test prints its figures (margins, dropped-case shares, the segmentation's
batch-order spread) before it asserts."""
from __future__ import annotations

import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assign_ref as AR  # noqa: E402
import diarize_ref as DR  # noqa: E402
import test_diarize_gpu as TG  # noqa: E402
import test_diarize_many_cpu as MC  # noqa: E402

PKG = "speaker-diarization-toolkit_amd"
dz = importlib.import_module(f"{PKG}.diarize")
seg = importlib.import_module(f"{PKG}.segmentation")
rn = importlib.import_module(f"{PKG}.resnet")
pytestmark = pytest.mark.gpu
RATE, CHUNK, F = 16000, 160000, 589


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).cuda()


# ------------------------------------------------------------------------------------------------ kernels, bit for bit
@pytest.mark.parametrize("step_s", [1.0, 2.5])
@pytest.mark.parametrize("maxsp", [None, 1, 0])
def test_reconstruct_grouped_bit_for_bit(engine, step_s, maxsp):
    """R = 5 (0 samples, 5 s, exactly 10 s, 23 s + 333 samples, 31 s), K_r in {0, 1, 3, 70}, labels with -1."""
    K_list = [3, 0, 1, 70, 3]
    n, starts, cls, labels, chunk_off, frame_off, cent_off = MC.reconstruct_case(step_s, K_list, 17)
    assert (labels == -1).any() and (labels >= 0).any()
    tab = dz.GroupTables(engine, chunk_off, frame_off, n, np.concatenate(starts)).set_clusters(cent_off, want_act=True)
    count, speakers, act = dz.diarize_reconstruct_grouped(engine, dev(cls), dev(labels), tab, maxsp, want_act=True)
    torch.cuda.synchronize()
    count, speakers, act = count.cpu().numpy(), speakers.cpu().numpy(), act.cpu().numpy()
    for r in range(len(n)):
        a, b, g0, g1 = int(chunk_off[r]), int(chunk_off[r + 1]), int(frame_off[r]), int(frame_off[r + 1])
        if a == b:
            assert g0 == g1
            continue
        K = max(K_list[r], 1)
        rc, rs, ract, _ = DR.reconstruct(cls[a:b], starts[r], labels[a:b], K, int(n[r]), maxsp)
        assert np.array_equal(count[g0:g1], rc) and np.array_equal(speakers[g0:g1], rs)
        assert np.array_equal(act[int(tab.act_off[r]):int(tab.act_off[r + 1])].reshape(g1 - g0, K), ract)


ASSIGN_SEED = {64: 3, 192: 3, 512: 3}      # seeds for which the reference alone keeps >= 95 % of the chunks (checked on the CPU; asserted below)


@pytest.fixture(scope="module")
def assign_refs():
    """The per-recording references of every (d, constrained), computed once."""
    out = {}
    for d in (64, 192, 512):
        E, info, cent, chunk_off, cent_off, per = MC.assign_cases(d, ASSIGN_SEED[d])
        out[d] = (E, info, cent, chunk_off, cent_off,
                  {c: [AR.assign(E_r, info_r, [], [], constrained=bool(c), cent=cent_r) for E_r, info_r, cent_r in per] for c in (0, 1)})
    return out


@pytest.mark.parametrize("d", [64, 192, 512])
@pytest.mark.parametrize("constrained", [0, 1])
def test_assign_grouped_against_the_reference_per_recording(engine, assign_refs, d, constrained):
    """C_r in {0, 1, 7, 40} x K_r in {0, 1, 2, 5, 70}, non-candidate rows NaN-filled; labels exact where the reference's decisive margin
    exceeds (3 d + 6) 2^-52, scores within fp32 rounding of the float64 cosine."""
    E, info, cent, chunk_off, cent_off, refs = assign_refs[d]
    assert np.isnan(E).any()
    tab = dz.GroupTables(engine, chunk_off, np.zeros_like(chunk_off), np.zeros(len(chunk_off) - 1, np.int64)).set_clusters(cent_off)
    labels, score = dz.diarize_assign_grouped(engine, dev(E), dev(info), dev(np.concatenate([cent, np.zeros((1, d))])), tab, bool(constrained))
    torch.cuda.synchronize()
    labels, score = labels.cpu().numpy(), score.cpu().numpy()
    assert not np.isnan(score).any()
    total = kept = 0
    err = 0.0
    for r, ref in enumerate(refs[constrained]):
        a, b = int(chunk_off[r]), int(chunk_off[r + 1])
        ok = ref["margin"] > (3 * d + 6) * 2.0 ** -52
        total, kept = total + int((ref["m"] > 0).sum()), kept + int(((ref["m"] > 0) & ok).sum())
        assert np.array_equal(labels[a:b][ok], ref["labels"][ok]), f"recording {r}"
        err = max(err, float(np.abs(score[a:b][ok] - ref["score"][ok]).max(initial=0.0)))
        assert np.array_equal(labels[a:b][ref["m"] == 0], np.full((int((ref["m"] == 0).sum()), 3), -1))
    print(f"assign grouped d={d} constrained={constrained}: chunks with candidates {total}, dropped for a margin <= (3 d + 6) 2^-52: {total - kept} "
          f"({(total - kept) / total:.4f}), max |score - float64 cosine| {err:.3e} (bound 2^-24 + 1e-12)")
    assert kept >= 0.95 * total
    assert err <= 2.0 ** -24 + 1e-12                                     # cosines are at most 1 in size: half an fp32 ulp of 1, and the float64 sum's own error


def test_fold_grouped_equals_fold_small_clusters_per_recording(engine):
    cases = MC.fold_cases(5)
    _, sizes, cl_off, eff, cent_off, ref, margins = MC.fold_tables(cases)
    print(f"fold grouped: least best-minus-second cosine of a small cluster in the reference {min(margins):.3e} (must exceed 1e-9)")
    assert min(margins) > 1e-9
    E = np.concatenate([c[0] for c in cases]).astype(np.float32)
    cut = np.concatenate([c[1].astype(np.int64) + int(cl_off[r]) for r, c in enumerate(cases)]).astype(np.int32)
    rows = np.arange(len(cut), dtype=np.int32)
    _, c64 = dz.diarize_centroids(engine, dev(E), dev(rows), dev(cut), int(cl_off[-1]))
    remap, out = dz.diarize_fold_grouped(engine, c64, sizes, cl_off, eff, cent_off, dev(cut))
    torch.cuda.synchronize()
    remap, out = remap.cpu().numpy(), out.cpu().numpy()
    assert np.array_equal(out, remap[cut])
    a = 0
    for r, (_, lab, _) in enumerate(cases):
        assert np.array_equal(out[a:a + len(lab)] - cent_off[r], ref[r]), f"recording {r}"
        a += len(lab)
    with pytest.raises(ValueError, match="cent_off"):
        dz.diarize_fold_grouped(engine, c64, sizes, cl_off, eff, cent_off + np.arange(len(cent_off)), dev(cut))


def test_first_seen_and_renumber_equal_order_by_appearance(engine):
    tabs, frame_off, cent_off = MC.speakers_case(2)
    K = int(cent_off[-1])
    rng = np.random.default_rng(0)
    chunk_off = MC.offsets([9, 4, 3, 20])
    labels = np.concatenate([rng.integers(-1, max(k, 1), (c, 3)) if k else np.full((c, 3), -1) for c, k in zip(np.diff(chunk_off), np.diff(cent_off))]).astype(np.int32)
    c32 = rng.standard_normal((K, 64)).astype(np.float32)
    c64 = rng.standard_normal((K, 64))
    n = np.array([0 if g == 0 else 495 + 270 * (g - 1) + 1 for g in np.diff(frame_off)], np.int64)
    tab = dz.GroupTables(engine, chunk_off, frame_off, n).set_clusters(cent_off)
    first = dz.diarize_first_seen(engine, dev(np.concatenate(tabs)), tab)
    lab_d = dev(labels)
    renum, o32, o64 = dz.diarize_renumber(engine, first, lab_d, dev(c32), dev(c64), tab)
    torch.cuda.synchronize()
    first, renum, lab2, o32, o64 = first.cpu().numpy(), renum.cpu().numpy(), lab_d.cpu().numpy(), o32.cpu().numpy(), o64.cpu().numpy()
    assert np.array_equal(first, dz.first_seen_host(np.concatenate(tabs), frame_off, cent_off))
    never = slot1 = 0
    for r, sp in enumerate(tabs):
        b, e = int(cent_off[r]), int(cent_off[r + 1])
        new = np.asarray(DR.order_by_appearance(sp, e - b), np.int64)
        assert np.array_equal(renum[b:e], new)
        lab = labels[int(chunk_off[r]):int(chunk_off[r + 1])]
        assert np.array_equal(lab2[int(chunk_off[r]):int(chunk_off[r + 1])], np.where(lab >= 0, new[np.maximum(lab, 0)] if e > b else -1, -1))
        if e > b:
            assert np.array_equal(o32[b:e], c32[b:e][np.argsort(new)]) and np.array_equal(o64[b:e], c64[b:e][np.argsort(new)])
        seen = first[b:e] != np.iinfo(np.int32).max
        never, slot1 = never + int((~seen).sum()), slot1 + int((first[b:e][seen] % 2 == 1).sum())
    assert never >= 3 and slot1 >= 1


# ------------------------------------------------------------------------------------------------ the front end on a packed buffer
def test_front_end_on_the_packed_buffer_equals_every_recording_alone(engine):
    """fbank_windows and Segmentation.forward over a packed buffer of three recordings (5 s, 12 s, 23 s) against the same chunks cut from each
    recording alone, in the same batch order."""
    rng = np.random.default_rng(4)
    recs = [np.clip(np.round(rng.normal(0, 0.1, n) * 32768), -32768, 32767).astype(np.int16) for n in (5 * RATE, 12 * RATE, 23 * RATE)]
    pack = dz.pack_recordings(recs, 1.0)
    Cn = int(pack.chunk_off[-1])
    buf, sp = dev(pack.samples), dev(pack.starts_packed)
    got = engine.fbank_windows(buf.data_ptr(), int(buf.numel()), sp.data_ptr(), Cn, CHUNK)
    alone = []
    for r, x in enumerate(recs):
        a, b = int(pack.chunk_off[r]), int(pack.chunk_off[r + 1])
        xd, sd = dev(x), dev(pack.starts_local[a:b])
        alone.append(engine.fbank_windows(xd.data_ptr(), len(x), sd.data_ptr(), b - a, CHUNK))
    torch.cuda.synchronize()
    assert torch.equal(got, torch.cat(alone)), "fbank_windows on the packed buffer differs from the recordings alone"
    model = seg.Segmentation(engine, seg.synthetic_weights(0))
    rows = np.stack([np.pad(x[s:s + CHUNK], (0, max(0, int(s) + CHUNK - len(x)))) for r, x in enumerate(recs)
                     for s in pack.starts_local[int(pack.chunk_off[r]):int(pack.chunk_off[r + 1])]])
    lp_rows = model.forward(dev(rows)).clone()                           # the same chunks, cut on the host from every recording alone, same batch order
    a = int(pack.chunk_off[2])
    lp_last = model.forward(dev(recs[2]), dev(pack.starts_local[a:])).clone()       # the last recording's chunks in a batch of their own
    lp_pack = model.forward(buf, sp).clone()
    torch.cuda.synchronize()
    spread = float((lp_rows[a:] - lp_last).abs().max())                  # two calls of the unchanged forward: is it batch-order invariant here?
    diff = float((lp_pack - lp_rows).abs().max())
    print(f"segmentation on the packed buffer: batch-order spread of the forward itself {spread:.3e} -> tolerance {2 * spread:.3e}; packed vs alone {diff:.3e}")
    if spread == 0.0:
        assert torch.equal(lp_pack, lp_rows)
    else:
        assert diff <= 2 * spread


# ------------------------------------------------------------------------------------------------ end to end
N_B = 23 * RATE + 333
N_C = 5 * RATE


def cls_for(n_samples, step_s):
    """scenario()'s class table for the first n_samples of its recording: the same layout, nobody speaks past the end."""
    st = seg.chunk_starts(n_samples, step_s)
    cls = np.zeros((len(st), F), np.uint8)
    single = {0: 1, 1: 2, 2: 3}
    pair = {frozenset((0, 1)): 4, frozenset((0, 2)): 5, frozenset((1, 2)): 6}
    for c in range(len(st)):
        local = {}
        for i in range(F):
            t = (int(st[c]) + 270 * i + 495) / RATE
            on = sorted({v for v, a, b in TG.LAYOUT if a <= t < b and t < n_samples / RATE})
            for v in on:
                local.setdefault(v, len(local))
            ids = {local[v] for v in on}
            cls[c, i] = 0 if not ids else single[next(iter(ids))] if len(ids) == 1 else pair[frozenset(ids)]
    return st, cls


@pytest.fixture(scope="module")
def weights():
    return rn.synthetic_weights(0)


@pytest.fixture(scope="module")
def net(engine, weights):
    return rn.ResNet34(engine, weights, precision=0)


@pytest.fixture(scope="module")
def recordings(weights):
    """A = scenario()'s 42 s, B = its first 23 s + 333 samples, C = its first 5 s, D = empty, with their class tables, and the CPU
    reference of each (B's chunks that start at A's starts and end before B's end are A's: their rows are reused)."""
    pcm, st, cls = TG.scenario()
    E_A, info_A = TG.reference_embeddings(weights, pcm, st, cls)
    e32, _ = TG.reference_embeddings(weights, pcm, st, cls, acc=torch.float32, chunks=[2, 9])
    ok = info_A[[2, 9]].reshape(-1, 4)[:, 3] != 0
    bound = TG.FACTOR * float(TG.one_cos(e32[ok], E_A.reshape(len(st), 3, -1)[[2, 9]].reshape(len(ok), -1)[ok]).max())
    recs = {"A": (pcm, st, cls, E_A, info_A)}
    for name, n in (("B", N_B), ("C", N_C)):
        x = pcm[:n]
        st_n, cls_n = cls_for(n, TG.STEP_S)
        same = [c for c in range(len(st_n)) if c < len(st) and st_n[c] == st[c] and np.array_equal(cls_n[c], cls[c]) and st_n[c] + CHUNK <= n]
        new = [c for c in range(len(st_n)) if c not in same]
        E_new, info_n = TG.reference_embeddings(weights, x, st_n, cls_n, chunks=new)
        _, info_n = DR.masks(cls_n, TG.T4_CHUNK)
        E_n = np.zeros((3 * len(st_n), E_A.shape[1]))
        for c in same:
            E_n[3 * c:3 * c + 3] = E_A[3 * c:3 * c + 3]
        for j, c in enumerate(new):
            E_n[3 * c:3 * c + 3] = E_new[3 * j:3 * j + 3]
        recs[name] = (x, st_n, cls_n, E_n, info_n)
    return recs, float(np.sqrt(2 * bound))


def margins_of(name, rec, move):
    """The reference pipeline of one recording and its decisive margins (the cut gap, and the constrained assignment's gap)."""
    x, st, cls, E, info = rec
    ref = DR.pipeline(cls, st, E, info, len(x), TG.E2E_THRESHOLD, TG.E2E_MIN_CLUSTER)
    cut_gap, cos_gap = TG.decisive_margins(ref, TG.E2E_THRESHOLD)
    con = AR.assign(E, info, ref["train"], ref["train_labels"], constrained=True)
    con_gap = float(con["margin"][con["m"] > 0].min()) if (con["m"] > 0).any() else np.inf
    print(f"e2e many, recording {name}: K={ref['K']} train={len(ref['train'])} cut gap {cut_gap:.3e} assignment gap {cos_gap:.3e} (each must exceed "
          f"{10 * move:.3e} = 10 x the row displacement of the GPU against the CPU reference); constrained gap {con_gap:.3e} (must exceed 1e-4)")
    assert cut_gap > 10 * move and cos_gap > 10 * move
    # run and run_many apply ONE kernel rule to embeddings of the same kernels in other batches: rows that moved by more than the 1e-6 allowed
    # on the centroids would fail that check itself, so 100 x that displacement decides the constrained matching between the two
    assert con_gap > 1e-4
    return ref


def same_result(a, b):
    assert np.array_equal(a.cls.cpu().numpy(), b.cls.cpu().numpy()) and np.array_equal(a.info, b.info) and np.array_equal(a.starts, b.starts)
    assert np.array_equal(a.labels, b.labels) and np.array_equal(a.count, b.count) and np.array_equal(a.speakers, b.speakers)
    assert a.turns == b.turns and a.n_speakers == b.n_speakers
    assert a.centroids.shape == b.centroids.shape and np.abs(a.centroids - b.centroids).max(initial=0.0) <= 1e-6


def test_run_many_equals_the_reference_and_run(engine, net, recordings, monkeypatch):
    recs, move = recordings
    refs = {k: margins_of(k, recs[k], move) for k in "ABC"}
    assert refs["A"]["K"] == 3
    D = np.zeros(0, np.int16)
    kw = dict(step_s=TG.STEP_S, threshold=TG.E2E_THRESHOLD, min_cluster_size=TG.E2E_MIN_CLUSTER)
    diar = dz.Diarizer(engine, None, net)
    lp = {k: TG.logp_of(recs[k][2]) for k in "ABC"}
    # against the CPU reference, as the single-recording end-to-end test does (unconstrained)
    many = diar.run_many([recs["A"][0], recs["B"][0], recs["C"][0], D], logp=[lp["A"], lp["B"], lp["C"], None], **kw)
    assert len(many) == 4 and many[3].turns == [] and many[3].n_speakers == 0 and many[3].cls is None and many[3].labels.shape == (0, 3)
    print(f"run_many: waits for the device per pack {diar.last_sync}")
    for k, res in zip("ABC", many):
        ref = refs[k]
        assert np.array_equal(res.cls.cpu().numpy(), recs[k][2]) and np.array_equal(res.info, recs[k][4])
        assert np.array_equal(res.labels, ref["labels"])
        assert np.array_equal(res.count, ref["count"]) and np.array_equal(res.speakers, ref["speakers"])
        assert res.turns == ref["turns"] and res.n_speakers == ref["K"]
    assert many[0].n_speakers == 3 and dz.to_rttm(many[0].turns, "rec") == DR.rttm(refs["A"]["turns"], "rec")
    # against run, recording by recording, constrained; then in reverse order and with batches of 5 chunks
    alone = {k: diar.run(recs[k][0], logp=lp[k], constrained=True, **kw) for k in "ABC"}
    con = diar.run_many([recs["A"][0], recs["B"][0], recs["C"][0], D], logp=[lp["A"], lp["B"], lp["C"], None], constrained=True, **kw)
    for k, res in zip("ABC", con):
        same_result(res, alone[k])
        assert res.scores is not None and np.abs(res.scores - alone[k].scores).max() <= 1e-6
    monkeypatch.setenv("SDK_DIARIZE_BATCH", "5")
    rev = diar.run_many([D, recs["C"][0], recs["B"][0], recs["A"][0]], logp=[None, lp["C"], lp["B"], lp["A"]], constrained=True, **kw)
    assert rev[0].turns == []
    for k, res in zip("CBA", rev[1:]):
        same_result(res, alone[k])
    monkeypatch.setenv("SDK_DIARIZE_PACK_SAMPLES", str(N_B + 2 * CHUNK))    # packs of one or two recordings
    split = diar.run_many([D, recs["C"][0], recs["B"][0], recs["A"][0]], logp=[None, lp["C"], lp["B"], lp["A"]], constrained=True, **kw)
    assert len(diar.last_sync) == 3
    for k, res in zip("CBA", split[1:]):
        same_result(res, alone[k])


def test_backend_diarize_many_with_the_models_own_logp(engine, monkeypatch):
    for k in ("SDK_MODEL", "SDK_NO_TORCH", "SDK_PRECISION", "SDK_RESNET_WEIGHTS", "SDK_SEGMENTATION_WEIGHTS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SDK_DIARIZE_BATCH", "5")
    be = importlib.import_module(f"{PKG}.backend").Backend()
    pcm, _, _ = TG.scenario()
    recs = [pcm[:N_B], pcm[20 * RATE:32 * RATE]]
    prec = be.engine().precision
    a = be.diarize_many(recs, step_s=1.0, threshold=0.5, min_cluster_size=2)
    b = be.diarize_many(recs, step_s=1.0, threshold=0.5, min_cluster_size=2)
    assert be.engine().precision == prec
    for x, ra, rb in zip(recs, a, b):
        assert ra.turns == rb.turns and np.array_equal(ra.labels, rb.labels) and np.array_equal(ra.speakers, rb.speakers)
        assert np.array_equal(ra.centroids, rb.centroids) and np.array_equal(ra.scores, rb.scores)
        cls = ra.cls.cpu().numpy()
        assert cls.shape == (len(seg.chunk_starts(len(x), 1.0)), F) and np.array_equal(ra.info, DR.masks(cls, TG.T4_CHUNK)[1])
        K = ra.n_speakers
        count, speakers, _, _ = DR.reconstruct(cls, ra.starts, ra.labels, max(K, 1), len(x))
        assert np.array_equal(ra.count, count) and np.array_equal(ra.speakers, speakers)
        assert ra.turns == DR.turns(speakers, K) and ra.centroids.shape == (K, 192)
        if K:
            assert np.allclose(np.linalg.norm(ra.centroids, axis=1), 1.0, atol=1e-5)
            assert DR.order_by_appearance(speakers, K) == list(range(K))
        print(f"own logp, many: {len(ra.starts)} chunks, K={K}, {len(ra.turns)} turns")
    v = be.diarize_many(recs, step_s=1.0, threshold=0.5, clustering="vbx", constrained=True)
    assert all(r.scores is not None and r.labels.shape == (len(r.starts), 3) for r in v)
    assert be.diarize_many([]) == []


def test_refusals_are_python_exceptions(engine, net):
    diar = dz.Diarizer(engine, None, net)
    x = np.zeros(12 * RATE, np.int16)
    Cn = len(seg.chunk_starts(len(x), 1.0))
    with pytest.raises(ValueError, match=r"one array per recording \(2\)"):
        diar.run_many([x, x], logp=[np.zeros((Cn, F, 7), np.float32)])
    with pytest.raises(ValueError, match=rf"recording 1: injected logp must be \[{Cn}, {F}, 7\]"):
        diar.run_many([x, x], logp=[np.zeros((Cn, F, 7), np.float32), np.zeros((Cn + 1, F, 7), np.float32)])
    with pytest.raises(ValueError, match=r"recording 1: .*65536 rows .*step_s"):
        diar.run_many([x, np.zeros(160000 + 160 * 21846, np.int16)], step_s=0.01)
    with pytest.raises(ValueError, match="clustering='spectral'"):
        diar.run_many([x], clustering="spectral")
    env = dict(os.environ, SDK_NO_TORCH="1")
    code = (f"import importlib, numpy as np\nbe = importlib.import_module('{PKG}.backend').Backend()\n"
            "try:\n    be.diarize_many([np.zeros(16000, np.int16)])\nexcept ValueError as e:\n    print('REFUSED:', e)\n")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert "REFUSED: diarize needs the torch engine: not available with SDK_NO_TORCH=1" in out.stdout, out.stdout + out.stderr
