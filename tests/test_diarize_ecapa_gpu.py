"""Diarization in the ECAPA space on the GPU: diarize.Diarizer on ecapa_diar.EcapaEmbedder with injected segmentation output (run, run_many
and a stream), the discrete outcomes against the host restatement of tests/diarize_ref.py applied to the embeddings the device produced (so
they do not hang on rounding), and the naming of a diarization's speakers from enrolled profiles through Backend.link_speakers."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import diarize_ref as DR
from conftest import sub
import stream_ref as SR
from test_diarize_gpu import RATE, STEP_S, logp_of, scenario        # the generated three-speaker recording of the ResNet34 e2e test

pytestmark = pytest.mark.gpu

dz = sub("diarize")
seg = sub("segmentation")
rn = sub("resnet")
ED = sub("ecapa_diar")
MIN_CLUSTER = 2
N40 = 40 * RATE


def _cut(pcm, cls, n):
    st = seg.chunk_starts(n, STEP_S)
    return pcm[:n], st, cls[:len(st)]


def _embeddings_of(d, pcm, st, cls):
    """the device's own unit embeddings of every chunk (rows that are not valid zeroed, as Diarizer.run reads them) and info"""
    eng = d.eng
    if eng.precision != d.embedder.precision:
        eng.set_precision(d.embedder.precision)
    rec = torch.from_numpy(pcm).to(eng.device)
    c, info, E = d._embed_all(rec, len(pcm), torch.from_numpy(st.astype(np.int32)).to(eng.device), torch.from_numpy(logp_of(cls)).to(eng.device))
    torch.cuda.synchronize()
    assert np.array_equal(c.cpu().numpy(), cls)
    E, info = E.cpu().numpy(), info.cpu().numpy()
    E[info.reshape(-1, 4)[:, 3] == 0] = 0.0
    return E, info


def _references(d, recs):
    """recs: [(pcm, st, cls)] -> (threshold, clearance, [reference pipeline result], [info]): ONE threshold for all recordings, the middle
    of the widest gap of their MERGED linkage heights (host restatement on the device's own embeddings) whose cut keeps two speakers or more
    in the first recording; the clearance is the distance of the threshold to the nearest merge height of ANY of the recordings."""
    emb = [_embeddings_of(d, *r) for r in recs]
    heights = np.sort(np.concatenate([DR.pipeline(cls, st, E, info, len(pcm), 0.5, MIN_CLUSTER)["Z"][:, 2] for (pcm, st, cls), (E, info) in zip(recs, emb)]))
    gaps = np.diff(heights)
    for i in np.argsort(-gaps):
        thr = float((heights[i] + heights[i + 1]) / 2)
        refs = [DR.pipeline(cls, st, E, info, len(pcm), thr, MIN_CLUSTER) for (pcm, st, cls), (E, info) in zip(recs, emb)]
        if refs[0]["K"] >= 2:
            return thr, float(gaps[i] / 2), refs, [info for _, info in emb]
    raise AssertionError("no cut of the reference linkages keeps two speakers in the first recording")


def _same(res, ref, info, cls):
    if getattr(res, "cls", None) is not None:
        assert np.array_equal(res.cls.cpu().numpy(), cls)
    assert np.array_equal(res.info, info)
    assert np.array_equal(res.labels, ref["labels"])
    assert np.array_equal(res.count, ref["count"]) and np.array_equal(res.speakers, ref["speakers"])
    assert res.turns == ref["turns"] and res.n_speakers == ref["K"]
    assert dz.to_rttm(res.turns, "rec") == DR.rttm(ref["turns"], "rec")


# the cut must not hang on rounding: merge heights are float64 sums over fp32 unit rows, and the rows of one chunk embedded in batches of
# different sizes differ by fp32 rounding at most (~1e-7 per row, a height moves by no more)
CLEARANCE = 1e-5


def test_run_and_run_many_on_injected_logp(engine):
    pcm, _, cls = scenario()
    pcm, st, cls = _cut(pcm, cls, N40)
    pcm2, st2, cls2 = _cut(pcm, cls, 25 * RATE)                          # the second recording: the first 25 s
    d = dz.Diarizer(engine, None, ED.EcapaEmbedder(engine, precision=0))
    assert d.embedder is d.resnet and d.embedder.last_map_frames(1001) == 1001
    thr, clear, (ref, ref2), (info, info2) = _references(d, [(pcm, st, cls), (pcm2, st2, cls2)])
    print(f"ECAPA diarization: {len(st)} + {len(st2)} chunks, threshold {thr:.4f} clear of every merge height of both linkages by {clear:.3e}, "
          f"K = {ref['K']} / {ref2['K']}, {len(ref['turns'])} / {len(ref2['turns'])} turns")
    assert clear > CLEARANCE
    res = d.run(pcm, step_s=STEP_S, threshold=thr, min_cluster_size=MIN_CLUSTER, logp=logp_of(cls))
    _same(res, ref, info, cls)
    assert res.centroids.shape == (ref["K"], 192) and res.centroids.shape[1] == 192
    assert np.allclose(np.linalg.norm(res.centroids, axis=1), 1.0, atol=1e-5)
    many = d.run_many([pcm, pcm2], step_s=STEP_S, threshold=thr, min_cluster_size=MIN_CLUSTER, logp=[logp_of(cls), logp_of(cls2)])
    _same(many[0], ref, info, cls)
    _same(many[1], ref2, info2, cls2)
    assert many[0].centroids.shape == (ref["K"], 192) and many[1].centroids.shape == (ref2["K"], 192)
    # (Diarizer.run leaves the engine in the embedder's contract by design; the caller restores it: the Backend test below checks that)


STREAM = dict(latency_s=STEP_S, capacity=6)                        # a stream's latency is at least its step
DELTAS = (0.6, 0.5, 0.7, 0.4, 0.8, 0.3, 0.9, 0.2)


def _run_bank(d, pcm, cls, delta):
    bank = d.open_streams(1, step_s=STEP_S, delta_new=delta, **STREAM)
    bank.keep_embeddings = True
    lp = logp_of(cls)
    k = bank.due(0, len(pcm))
    ups = bank.push([pcm], [lp[:k]])
    res = bank.finish(0, lp[k:k + 1] if k < len(cls) else None)
    E, kept = bank.embeddings(0)
    assert np.array_equal(kept, cls)
    return res, ups, E


def test_stream_pushed_then_finished_equals_the_reference(engine):
    """one stream on the ECAPA embedder (masks at T4 = T = 1001): labels, count, speakers, turns and RTTM equal tests/stream_ref.py applied
    to the embeddings the bank itself produced; delta_new is the first of DELTAS at which the reference decides every step with a margin"""
    pcm, _, cls = scenario()
    pcm, st, cls = _cut(pcm, cls, N40)
    d = dz.Diarizer(engine, None, ED.EcapaEmbedder(engine, precision=0))
    hop, latency = int(round(STEP_S * RATE)), int(round(STREAM["latency_s"] * RATE))
    info = dz.masks_host(cls, 1001)[1]
    _, _, E0 = _run_bank(d, pcm, cls, DELTAS[0])
    delta = None
    for dl in DELTAS:                                                    # chosen on the reference alone
        r = SR.run_stream(E0, info, cls, st, len(pcm), STREAM["capacity"], hop, latency, dl)
        if r["ref"].margin > 1e-4 and r["K"] >= 2:
            delta = dl
            break
    assert delta is not None, "no delta_new at which the reference decides every step with a margin"
    res, ups, E = _run_bank(d, pcm, cls, delta)
    assert np.array_equal(res.info, info) and np.array_equal(res.starts, st)
    ref = SR.run_stream(E, res.info, cls, st, len(pcm), STREAM["capacity"], hop, latency, delta)
    print(f"ECAPA stream: delta_new {delta} K = {ref['K']} margin {ref['ref'].margin:.3e} labels {res.labels.tolist()}")
    assert ref["ref"].margin > 1e-6 and ref["K"] >= 2                    # as tests/test_stream_gpu.py: fp32 rows of different batch sizes differ by far less
    assert np.array_equal(res.labels, ref["labels"]) and res.n_speakers == ref["K"]
    assert np.array_equal(res.count, ref["count"]) and np.array_equal(res.speakers, ref["speakers"])
    assert np.abs(res.scores - ref["score"]).max() <= 1e-6
    turns = dz.turns_from_frames(ref["speakers"], ref["K"])
    assert res.turns == turns and dz.to_rttm(res.turns, "rec") == DR.rttm(turns, "rec")
    assert res.centroids.shape == (ref["K"], 192)
    emitted = np.concatenate([u.speakers for u in ups])
    assert np.array_equal(emitted, res.speakers[:len(emitted)])


ENV = ("SDK_MODEL", "SDK_DIARIZE_MODEL", "SDK_NO_TORCH", "SDK_PRECISION", "SDK_RESNET_WEIGHTS", "SDK_SEGMENTATION_WEIGHTS", "SDK_COHORT", "SDK_COHORT_THRESHOLD")


def test_link_speakers_names_a_diarization_from_enrolled_profiles(engine, tmp_path, monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SPEAKERS_EMBEDDINGS_DIR", str(tmp_path / "store"))
    monkeypatch.setenv("SDK_CACHE_DIR", str(tmp_path / "cache"))
    monkeypatch.setenv("SDK_MODEL", "ecapa")
    monkeypatch.setenv("SDK_DIARIZE_MODEL", "ecapa")
    store = sub("store")
    be = sub("backend").Backend()
    prec = be.engine().precision
    d = be.diarizer()
    assert isinstance(d.embedder, ED.EcapaEmbedder) and d.embedder.eng is be.engine()
    pcm, _, cls = scenario()
    pcm, st, cls = _cut(pcm, cls, N40)
    thr, clear, (ref,), _ = _references(d, [(pcm, st, cls)])
    assert clear > CLEARANCE
    res = be.diarize(pcm, step_s=STEP_S, threshold=thr, min_cluster_size=MIN_CLUSTER, logp=logp_of(cls))
    assert be.engine().precision == prec, "the engine's precision is what it was"
    assert res.n_speakers == ref["K"] >= 2 and res.centroids.shape[1] == 192
    who = 1
    prof = {"id": "alice", "embeddings": {be.name: [{"id": "emb-alice", "external_id": store.save_vector(res.centroids[who]), "model_version": be.model_version,
                                                       "trust_level": "high"}]}}
    cc = res.centroids.astype(np.float64)
    dist = 1.0 - cc @ cc.T + 2.0 * np.eye(len(cc))
    lthr = float(dist.min()) / 2                                        # under every distance between two speakers, cosine or Euclidean: only the profile joins its centroid
    assert lthr > 1e-6
    links = be.link_speakers([res], threshold=lthr, candidates=[prof])
    g = int(links.ids[0][who])
    print(f"link_speakers: ids {links.ids[0].tolist()} names {links.names}")
    assert links.names[g] == "alice"
    assert [n for i, n in enumerate(links.names) if i != g] == [None] * (links.n_global - 1)
    # the same call with SDK_DIARIZE_MODEL unset is still refused, and the message names both ways
    monkeypatch.delenv("SDK_DIARIZE_MODEL")
    be2 = sub("backend").Backend()
    with pytest.raises(ValueError, match=r"link_speakers: candidates.*SDK_MODEL=resnet34, or with SDK_MODEL=ecapa and SDK_DIARIZE_MODEL=ecapa"):
        be2.link_speakers([res], threshold=lthr, candidates=[prof])


def test_default_diarizer_is_unchanged(engine, monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    be = sub("backend").Backend()
    assert be.diarize_model == "resnet34"
    assert isinstance(be.diarizer().resnet, rn.ResNet34) and be.diarizer().embedder is be.diarizer().resnet
