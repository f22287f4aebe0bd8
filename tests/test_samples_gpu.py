"""GPU checks of speaker samples (csrc/samples.hip, samples.py): sdk_samples_runs's run_off and rows bit for bit against the per-frame walk
of tests/samples_ref.py on every edge pack - the rule's cases and the scan's widths (wave, workgroup, per-workgroup span) - and on seeded
random packs, twice with equal bytes; sdk_samples_score against the math.fsum reference within 1e-12; the refusals; then
backend.speaker_samples and write_samples on the generated audio of tests/test_diarize_gpu.py."""
from __future__ import annotations

import functools
import wave
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import samples_ref as SR
import test_diarize_gpu as TG
from conftest import sub

sm = sub("samples")
ops_score = sub("ops_score")
LIB = sub("_lib")
pytestmark = pytest.mark.gpu

PACKS = SR.edge_packs()


def device_pack(engine, gap, min_fr, recs):
    """sdk_samples_runs on a pack -> (run_off [R + 1], rows [N, 4]) as the library wrote them."""
    from importlib import import_module
    GroupTables = import_module(sm.__package__ + ".diarize_ops").GroupTables
    G_r = [len(sp) for sp, _ in recs]
    tab = GroupTables(engine, np.zeros(len(recs) + 1, np.int64), np.concatenate([[0], np.cumsum(G_r)]), [270 * g + 226 if g else 0 for g in G_r])
    tab.set_clusters(np.concatenate([[0], np.cumsum([K for _, K in recs])]))
    sp_d = torch.from_numpy(np.concatenate([np.asarray(sp, np.int32).reshape(-1, 2) for sp, _ in recs])).to(engine.device)
    run_off, rows = ops_score.samples_runs(engine, sp_d, tab.frame_off_d, tab.cent_off_d, max(K for _, K in recs), gap, min_fr)
    run_off = run_off.cpu().numpy()
    return run_off, rows[:int(run_off[-1])].cpu().numpy()


@functools.lru_cache(maxsize=None)
def reference(name):
    gap, min_fr, recs = PACKS[name] if isinstance(name, str) else SR.random_pack(name)
    return SR.pack_ref(gap, min_fr, recs)


@pytest.mark.parametrize("name", sorted(PACKS))
def test_runs_bit_for_bit_on_every_edge(engine, name):
    gap, min_fr, recs = PACKS[name]
    assert ops_score.SAMPLES_SCAN_SPAN == SR.SPAN
    got_off, got = device_pack(engine, gap, min_fr, recs)
    want_off, want = reference(name)
    assert got_off.dtype == np.int32 and np.array_equal(got_off, want_off), (name, got_off.tolist(), want_off.tolist())
    assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (name, np.argwhere(got != want)[:4].tolist())
    # the pack through samples.runs, in seconds: the same rows, split by recording
    per = sm.runs(engine, [SimpleNamespace(speakers=sp, n_speakers=K) for sp, K in recs], (min_fr * 270 - 100) / 16000 if min_fr > 1 else 0.0, gap * 270 / 16000)
    assert [len(p) for p in per] == np.diff(want_off).tolist() and np.array_equal(np.concatenate(per), want)


@pytest.mark.parametrize("seed", [21, 22, 23])
def test_runs_bit_for_bit_on_random_packs_and_twice_the_same_bytes(engine, seed):
    gap, min_fr, recs = SR.random_pack(seed)
    (off_a, rows_a), (off_b, rows_b) = device_pack(engine, gap, min_fr, recs), device_pack(engine, gap, min_fr, recs)
    want_off, want = reference(seed)
    assert np.array_equal(off_a, want_off) and np.array_equal(rows_a, want) and len(want) > 0, (seed, np.argwhere(rows_a != want)[:4].tolist())
    assert off_a.tobytes() == off_b.tobytes() and rows_a.tobytes() == rows_b.tobytes()


@pytest.mark.parametrize("d", sorted(SR.SCORE_CASES))
def test_scores_against_float64(engine, d):
    """own, rival and mean within 1e-12 of the math.fsum reference (unit-scale float64 sums at d <= 512 carry about d 2^-53 times a small
    constant, 1e-13: 1e-12 leaves a decade); rival_speaker, windows and alone equal; two runs the same bytes.
    d = 320 and 448: a second column live for a part of the workgroup only.  Checked on the CPU (tests/test_samples_cpu.py prints them): least
    rest_ratio 0.424 and 0.427 (0.1 asked), least rival_gap 5.2e-3 and 1.7e-3 (1e-9 asked), 2 alone, 1 empty and 4 rival-less clips each;
    without the columns 256.. the reference names other rivals and its scores move by more than 1e11 x the 1e-12 bound."""
    E, clip_off, clip_spk, spk_off = SR.score_case(*SR.SCORE_CASES[d])
    want = SR.score_ref(E, clip_off, clip_spk, spk_off)
    # the inputs keep every decision away from rounding, on the reference alone, for every clip
    print(f"samples_score d={d}: least rest_ratio {want['rest_ratio'][want['alone'] == 0].min():.3e} (0.1 asked), least rival_gap {want['rival_gap'].min():.3e} "
          f"(1e-9 asked); alone {int(want['alone'].sum())}, empty {int((want['windows'] == 0).sum())}, rival-less {int((want['rival_speaker'] == -1).sum())}")
    assert (want["rest_ratio"][want["alone"] == 0] >= 0.1).all() and (want["rival_gap"] > 1e-9).all()
    assert want["alone"].sum() >= 2 and (want["windows"] == 0).sum() == 1 and (want["rival_speaker"] == -1).sum() >= 4
    if d > 256:
        SR.second_column_weight(f"samples_score d={d}", E, clip_off, clip_spk, spk_off, want)
    E_d = torch.from_numpy(E).to(engine.device)
    mean, out_f, out_i = sm.score(engine, E_d, clip_off, clip_spk, spk_off)
    err = (float(np.abs(mean - want["mean"]).max()), float(np.abs(out_f[:, 0] - want["own"]).max()), float(np.abs(out_f[:, 1] - want["rival"]).max()))
    print(f"samples_score d={d}: W={len(E)} M={len(clip_spk)} S={int(spk_off[-1])}; max |mean|, |own|, |rival| error {err[0]:.2e} {err[1]:.2e} {err[2]:.2e}; "
          f"worst / the 1e-12 bound {max(err) / 1e-12:.4f}")
    assert max(err) <= 1e-12
    assert np.array_equal(out_i[:, 0], want["rival_speaker"]) and np.array_equal(out_i[:, 1], want["windows"]) and np.array_equal(out_i[:, 2], want["alone"])
    again = sm.score(engine, E_d, clip_off, clip_spk, spk_off)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((mean, out_f, out_i), again))
    host = sm.score_host(E, clip_off, clip_spk, spk_off)
    assert np.abs(host[1] - out_f).max() <= 1e-12 and np.array_equal(host[2], out_i)


def test_refusals_are_exceptions_not_faults(engine):
    dev = engine.device
    up = lambda a, t=np.int32: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(t))).to(dev)  # noqa: E731
    sp, frame_off = up(np.zeros((10, 2))), up([0, 10])
    with pytest.raises(ValueError, match="1025 hypothesis speakers"):
        sm.runs(engine, [SimpleNamespace(speakers=np.zeros((10, 2), np.int32), n_speakers=1025)])
    with pytest.raises(ValueError, match="at most 1024"):
        ops_score.samples_runs(engine, sp, frame_off, up([0, 1025]), 1025, 59, 30)
    with pytest.raises(ValueError, match="must be a contiguous int32 device tensor"):
        ops_score.samples_runs(engine, sp.cpu(), frame_off, up([0, 1]), 1, 59, 30)
    with pytest.raises(ValueError, match="min_frames=0"):
        ops_score.samples_runs(engine, sp, frame_off, up([0, 1]), 1, 59, 0)
    # the library refuses a 1025th speaker and a short row table on its own, before any launch
    run_off = torch.full((2,), -7, dtype=torch.int32, device=dev)
    rows = torch.full((10, 4), -7, dtype=torch.int32, device=dev)
    ws = torch.empty(engine.lib.sdk_samples_runs_workspace_bytes(10), dtype=torch.uint8, device=dev)
    cent_off = up([0, 1])
    args = lambda max_hyp, cap: (engine.ctx, sp.data_ptr(), frame_off.data_ptr(), cent_off.data_ptr(), 1, 10, max_hyp, 59, 1, run_off.data_ptr(),  # noqa: E731
                                 rows.data_ptr(), cap, ws.data_ptr(), ws.numel(), None)
    rc = engine.lib.sdk_samples_runs(*args(1025, 10))
    assert rc != 0 and b"at most 1024" in engine.lib.sdk_last_error()
    with pytest.raises(LIB.SdkError, match="at most 1024"):
        LIB.check(rc, "sdk_samples_runs")
    assert engine.lib.sdk_samples_runs(*args(1, 9)) != 0 and b"rows_cap=9" in engine.lib.sdk_last_error()
    torch.cuda.synchronize()
    assert (run_off.cpu().numpy() == -7).all() and (rows.cpu().numpy() == -7).all()
    # scores: a width that is no multiple of 64, a width past 512, host memory, tables that do not fit
    E = torch.zeros((4, 64), dtype=torch.float32, device=dev)
    for bad in (96, 576):
        with pytest.raises(ValueError, match=f"d={bad} not supported"):
            ops_score.samples_score(engine, torch.zeros((4, bad), dtype=torch.float32, device=dev), up([0, 4]), up([0]), up([0, 1]), 1)
    with pytest.raises(ValueError, match="must be a contiguous fp32 device tensor"):
        ops_score.samples_score(engine, E.cpu(), up([0, 4]), up([0]), up([0, 1]), 1)
    with pytest.raises(ValueError, match="clip_spk must be a contiguous int32 device tensor"):
        ops_score.samples_score(engine, E, up([0, 4]), up([0, 0]), up([0, 1]), 1)
    with pytest.raises(ValueError, match="ascending offsets"):
        sm.score(engine, E, [0, 5], [0], [0, 1])
    with pytest.raises(ValueError, match=r"clip_spk must lie in \[0, 1\)"):
        sm.score(engine, E, [0, 4], [1], [0, 1])
    assert engine.lib.sdk_samples_score_workspace_bytes(1, 1, 96) == 0 and b"multiple of 64" in engine.lib.sdk_last_error()
    # a clip of nobody and offsets past E are read safely by the library itself: no score, no row outside E
    mean, out_f, out_i = ops_score.samples_score(engine, E + 1.0, up([0, 9]), up([5]), up([0, 1]), 1)
    assert out_f.cpu().numpy().tolist() == [[0.0, 0.0]] and out_i.cpu().numpy().tolist() == [[-1, 4, 1]] and not mean.cpu().numpy().any()


# ------------------------------------------------------------------------------------------------ end to end
SECONDS = 23                          # tests/test_diarize_gpu.py's shortest diarized recording: the first 23 s and 333 samples of its scenario


@pytest.fixture(scope="module")
def diarized(engine):
    """The recording, the backend and its diarization, made once: the scenario's first two voices with the class table of its layout injected
    (synthetic weights: the segmentation model's own output is noise), so the speakers table has long solo stretches."""
    import os
    saved = {k: os.environ.pop(k, None) for k in ("SDK_MODEL", "SDK_NO_TORCH", "SDK_PRECISION", "SDK_RESNET_WEIGHTS", "SDK_SEGMENTATION_WEIGHTS", "SDK_DIARIZE_MODEL")}
    saved["SDK_DIARIZE_BATCH"] = os.environ.get("SDK_DIARIZE_BATCH")
    os.environ["SDK_DIARIZE_BATCH"] = "5"
    try:
        bk = sub("backend")
        be = bk.Backend()
        pcm, _, _ = TG.scenario()
        pcm = pcm[:SECONDS * TG.RATE + 333]
        st = TG.seg.chunk_starts(len(pcm), TG.STEP_S)
        cls = np.zeros((len(st), TG.F), np.uint8)
        for c in range(len(st)):                                      # the scenario's own labelling, on this length's chunks
            local = {}
            for i in range(TG.F):
                t = (int(st[c]) + 270 * i + 495) / TG.RATE
                on = sorted({v for v, a, b in TG.LAYOUT if a <= t < b})
                for v in on:
                    local.setdefault(v, len(local))
                ids = sorted({local[v] for v in on})
                cls[c, i] = 0 if not ids else ids[0] + 1 if len(ids) == 1 else {(0, 1): 4, (0, 2): 5, (1, 2): 6}[tuple(ids)]
        result = be.diarize(pcm, step_s=TG.STEP_S, threshold=TG.E2E_THRESHOLD, min_cluster_size=TG.E2E_MIN_CLUSTER, logp=TG.logp_of(cls))
        yield bk, be, pcm, result
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def check_inside_solo_frames(result, k, a, b, gap):
    """Every frame whose samples [270 g + 360, 270 g + 630) meet the clip [a, b) is solo for k or silent, no more than gap silent in a row."""
    kinds = [SR.kind_of(e, result.n_speakers) for e in np.asarray(result.speakers).tolist()]
    silent = 0
    for g in range((a - 360) // 270, (b - 1 - 360) // 270 + 1):
        assert kinds[g] in (k, -1), (k, a, b, g, kinds[g])
        silent = silent + 1 if kinds[g] == -1 else 0
        assert silent <= gap


def test_speaker_samples_end_to_end(engine, diarized, tmp_path):
    bk, be, pcm, result = diarized
    K = result.n_speakers
    runs = SR.runs_ref(result.speakers, K, 59, 30)
    assert K >= 1 and len(runs) >= 2
    got = bk.speaker_samples(be, result, pcm, max_clip_s=3.0)
    assert isinstance(got, dict) and got and set(got) <= set(runs[:, 0].tolist())
    # every clip is a candidate: min_margin below any margin
    every = bk.speaker_samples(be, [result], [pcm], max_clip_s=3.0, min_margin=-3.0)
    assert isinstance(every, list) and len(every) == 1 and set(every[0]) == set(runs[:, 0].tolist())
    for k, lst in every[0].items():
        key = [(s.alone, -s.own, -s.solo_s, s.start_s) for s in lst]
        assert key == sorted(key)                                                       # the order of the rule
        for s in lst:
            a, b = int(round(s.start_s * 16000)), int(round(s.end_s * 16000))
            assert s.speaker == k and s.recording == 0 and s.start_s < s.end_s and b - a >= 8000 and b - a <= 48000
            check_inside_solo_frames(result, k, a, b, 59)
            assert s.alone or -1.0 - 1e-12 <= s.own <= 1.0 + 1e-12
            assert s.embedding.dtype == np.float32 and abs(float(np.linalg.norm(s.embedding.astype(np.float64))) - 1.0) < 1e-6
        assert all(s.alone or s.own - s.rival >= 0.0 for s in got.get(k, []))
    flat = sorted((s for lst in every[0].values() for s in lst), key=lambda s: s.start_s)
    clips = sm.cut_clips(runs, len(pcm), 3.0)
    assert [(s.speaker, int(round(s.start_s * 16000)), int(round(s.end_s * 16000))) for s in flat] == [tuple(c[:3]) for c in clips.tolist()]
    # the scores are score_host's on the embeddings of the same ranges, and the returned embeddings are embed_ranges's clip means: the
    # same ranges in the same order go through the same launches, and the forward is deterministic - equal bytes
    ranges = [(s.start_s, s.end_s) for s in flat]
    E, _, _, wins, dropped = be.embed_ranges(pcm, ranges)
    assert not dropped
    counts = np.bincount([ri for ri, _, _ in wins], minlength=len(flat))
    off = np.concatenate([[0], np.cumsum(counts)])
    emb = sm.clip_embeddings(E, np.stack([off[:-1], off[1:]], 1))
    assert emb.tobytes() == np.stack([s.embedding for s in flat]).tobytes()
    _, out_f, out_i = sm.score_host(E.cpu().numpy(), off, [s.speaker for s in flat], [0, K])
    assert np.abs(out_f[:, 0] - [s.own for s in flat]).max() <= 1e-12 and np.abs(out_f[:, 1] - [s.rival for s in flat]).max() <= 1e-12
    assert out_i[:, 0].tolist() == [s.rival_speaker for s in flat] and out_i[:, 2].astype(bool).tolist() == [s.alone for s in flat]
    # the pairs go to enroll_speaker's segments= as they are: the windows it would cut are those that were scored
    assert len(sub("wav").range_starts(len(pcm), ranges, hop_s=be.hop_s)[1]) == len(wins)
    paths = bk.write_samples(tmp_path, every[0], pcm)
    assert len(paths) == len(flat)
    by_speaker = {k: iter(lst) for k, lst in every[0].items()}
    for p in paths:
        s = next(by_speaker[int(p.parent.name[1:]) - 1])
        with wave.open(str(p), "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 16000)
            assert w.getnframes() == int(round(s.end_s * 16000)) - int(round(s.start_s * 16000))
    print(f"e2e: K={K}, {len(runs)} runs, {len(flat)} clips, kept at margin 0: { {k: len(v) for k, v in got.items()} }, "
          f"margins {[round(s.own - s.rival, 3) for s in flat]}")
