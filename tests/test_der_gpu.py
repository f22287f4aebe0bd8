"""GPU checks of the diarization error rate (csrc/score.hip, score.py): sdk_score_reference, sdk_score_cooccur and sdk_score_map alone, bit for bit
against tests/der_ref.py on packs of generated references and hypotheses, then Diarizer.score and Diarizer.sweep on the 42-s scenario of
tests/test_diarize_gpu.py.  Every comparison is integer equality."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import der_ref as DRF
import test_diarize_gpu as TG
from conftest import sub

sc = sub("score")
dz = sub("diarize")
seg = sub("segmentation")
LIB = sub("_lib")
pytestmark = pytest.mark.gpu

RATE = 16000
# 0 samples; 400 samples (no frame); 496 samples (one frame); 5 s; 23 s + 333 samples; 31 s; 60 s.  The packed grid has 1 + 295 + 1363 + 1836 +
# 3554 = 7049 frames: sdk_score_cooccur's workgroups take 4096, so the 60-s recording straddles a workgroup boundary and the first workgroup
# serves five recordings.
N_SAMPLES = [0, 400, 496, 5 * RATE, 23 * RATE + 333, 31 * RATE, 60 * RATE]
S_SETS = [(1, 3, 1, 3, 64, 1, 3), (0, 64, 0, 64, 3, 0, 64), (64, 0, 3, 1, 0, 3, 1)]
K_SETS = [(3, 1, 1, 64, 3, 0, 3), (0, 3, 3, 1, 64, 3, 64), (1, 0, 0, 3, 1, 64, 1)]


def tables(engine, n_samples, K_r=None):
    G_r = [dz.global_frames(n) for n in n_samples]
    tab = dz.GroupTables(engine, np.zeros(len(n_samples) + 1, np.int64), np.concatenate([[0], np.cumsum(G_r)]), n_samples)
    if K_r is not None:
        tab.set_clusters(np.concatenate([[0], np.cumsum(K_r)]))
    return tab


@functools.lru_cache(maxsize=None)
def pack_case(which: int):
    """One pack: (reference turn lists, speakers tables) for S_SETS[which] / K_SETS[which], computed once."""
    rng = np.random.default_rng(700 + which)
    refs = [DRF.random_turns(rng, S, n) for S, n in zip(S_SETS[which], N_SAMPLES)]
    hyps = [DRF.random_speakers(rng, dz.global_frames(n), K) for K, n in zip(K_SETS[which], N_SAMPLES)]
    return refs, hyps


@functools.lru_cache(maxsize=None)
def restated(which: int, collar_s: float, skip: bool):
    refs, hyps = pack_case(which)
    return [DRF.der_ref(h, n, t, collar_s, skip, K=K) for h, n, t, K in zip(hyps, N_SAMPLES, refs, K_SETS[which])]


@pytest.mark.parametrize("collar_s,skip", [(0.0, False), (0.25, False), (0.0, True), (0.25, True)])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_reference_masks_bit_for_bit(engine, which, collar_s, skip):
    refs, _ = pack_case(which)
    tab = tables(engine, N_SAMPLES)
    ref = sc.rasterise_references(engine, tab, refs, collar_s, skip)
    mask, scored = ref.ref_mask.cpu().numpy().view(np.uint64), ref.scored.cpu().numpy()
    assert mask.shape == (tab.G,) and scored.shape == (tab.G,)
    for r, want in enumerate(restated(which, collar_s, skip)):
        g0, g1 = int(tab.frame_off[r]), int(tab.frame_off[r + 1])
        assert ref.names[r] == want["names"] and len(want["names"]) == S_SETS[which][r]
        assert [int(v) for v in mask[g0:g1]] == want["mask"], (which, r)
        assert [bool(v) for v in scored[g0:g1]] == want["scored_frames"], (which, r)


@pytest.mark.parametrize("collar_s,skip", [(0.0, False), (0.25, True)])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_cooccurrence_and_tallies_bit_for_bit(engine, which, collar_s, skip):
    refs, hyps = pack_case(which)
    for h in hyps:                                             # rows of all three kinds wherever a recording has frames and two speakers
        if len(h) > 8 and h.max() >= 1:
            assert ((h[:, 0] < 0) & (h[:, 1] < 0)).any() and ((h[:, 0] >= 0) & (h[:, 1] < 0)).any() and (h[:, 1] >= 0).any()
    tab = tables(engine, N_SAMPLES, K_SETS[which])
    got = sc.score_grouped(engine, torch.from_numpy(np.concatenate(hyps)).to(engine.device), tab, refs, collar_s, skip)
    again = sc.score_grouped(engine, torch.from_numpy(np.concatenate(hyps)).to(engine.device), tab, refs, collar_s, skip)
    for r, (res, want) in enumerate(zip(got, restated(which, collar_s, skip))):
        assert res.co.shape == (S_SETS[which][r], K_SETS[which][r]) and np.array_equal(res.co, want["co"]), (which, r)
        assert (res.scored, res.total, res.missed, res.false_alarm) == (want["scored"], want["total"], want["missed"], want["false_alarm"]), (which, r)
        assert (res.correct, res.confusion) == (want["correct"], want["confusion"]) and res.der == want["der"], (which, r)
        m = [res.mapping[nm] for nm in want["names"]]
        used = [j for j in m if j >= 0]
        assert len(set(used)) == len(used) and all(res.co[i, j] > 0 for i, j in enumerate(m) if j >= 0)
        assert sum(int(res.co[i, j]) for i, j in enumerate(m) if j >= 0) == res.correct
        assert np.array_equal(again[r].co, res.co) and again[r].mapping == res.mapping and again[r].correct == res.correct
    print(f"pack {which} collar {collar_s} skip {skip}: pooled {sc.pool(got)}")


SHAPES = [(1, 1), (1, 64), (64, 1), (3, 5), (37, 64), (64, 64)]


def test_assignment_is_exact(engine):
    rng = np.random.default_rng(26)
    cos = []
    for S, K in SHAPES:
        cos += [rng.integers(0, 1 << 20, (S, K)), rng.integers(0, 2, (S, K)), np.zeros((S, K), np.int64), rng.integers(0, 1 << 30, (S, K))]
        cos[-1][rng.integers(0, S), rng.integers(0, K)] = (1 << 30) - 1
    R = len(cos)
    ref_off = np.concatenate([[0], np.cumsum([c.shape[0] for c in cos])])
    cent_off = np.concatenate([[0], np.cumsum([c.shape[1] for c in cos])])
    co_off = np.concatenate([[0], np.cumsum([c.size for c in cos])]).astype(np.int64)
    dev = engine.device
    up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).astype(t)).to(dev)  # noqa: E731
    co_d, ref_d, cent_d, off_d = up(np.concatenate([c.reshape(-1) for c in cos]), np.int32), up(ref_off, np.int32), up(cent_off, np.int32), up(co_off, np.int64)
    mapping = torch.full((int(ref_off[-1]),), -7, dtype=torch.int32, device=dev)
    correct = torch.full((R,), -7, dtype=torch.int64, device=dev)
    # the library's own refusal of more than 64 speakers comes before any launch
    assert engine.lib.sdk_score_map(engine.ctx, co_d.data_ptr(), ref_d.data_ptr(), cent_d.data_ptr(), off_d.data_ptr(), R, 65, 64, mapping.data_ptr(), correct.data_ptr(),
                                    None) != 0 and b"at most 64" in engine.lib.sdk_last_error()
    LIB.check(engine.lib.sdk_score_map(engine.ctx, co_d.data_ptr(), ref_d.data_ptr(), cent_d.data_ptr(), off_d.data_ptr(), R, 64, 64, mapping.data_ptr(),
                                       correct.data_ptr(), None), "sdk_score_map")
    mapping, correct = mapping.cpu().numpy(), correct.cpu().numpy()
    for r, co in enumerate(cos):
        rows, cols = linear_sum_assignment(co, maximize=True)
        assert int(correct[r]) == int(co[rows, cols].sum()), (r, co.shape)
        m = mapping[int(ref_off[r]):int(ref_off[r + 1])]
        assert ((m >= -1) & (m < co.shape[1])).all()
        used = m[m >= 0]
        assert len(set(used.tolist())) == len(used), (r, co.shape)
        assert all(co[i, j] > 0 for i, j in enumerate(m) if j >= 0)
        assert sum(int(co[i, j]) for i, j in enumerate(m) if j >= 0) == int(correct[r])


# ------------------------------------------------------------------------------------------------ end to end
# Thresholds, chosen on the CPU reference pipeline (tests/diarize_ref.py on the scenario's reference embeddings, min_cluster_size 2): its linkage
# has heights 0.052 .. 0.608; cut at 0.2 (between the heights 0.182 and 0.240) it keeps 7 clusters, an over-split; at the default 0.7046 and
# at 10.0 (above every height: distances of unit rows are at most 2) it keeps one.  A threshold below 0.1 would NOT over-split: every cluster
# is then smaller than min_cluster_size and the fold sends all rows to one.
THRESHOLDS = [0.2, 0.7045654963945799, 10.0]
SHORT = 20 * RATE


def scenario_cls(n_samples: int):
    """TG.scenario's class table for the first n_samples of its recording."""
    st = seg.chunk_starts(n_samples, TG.STEP_S)
    cls = np.zeros((len(st), TG.F), np.uint8)
    single = {0: 1, 1: 2, 2: 3}
    pair = {frozenset((0, 1)): 4, frozenset((0, 2)): 5, frozenset((1, 2)): 6}
    for c in range(len(st)):
        local = {}
        for i in range(TG.F):
            t = (int(st[c]) + 270 * i + 495) / RATE
            on = sorted({v for v, a, b in TG.LAYOUT if a <= t < b and int(st[c]) + 270 * i + 495 < n_samples})
            for v in on:
                local.setdefault(v, len(local))
            ids = {local[v] for v in on}
            cls[c, i] = 0 if not ids else single[next(iter(ids))] if len(ids) == 1 else pair[frozenset(ids)]
    return cls


def tallies_of(r):
    return (r.scored, r.total, r.missed, r.false_alarm, r.confusion, r.correct)


def test_score_and_sweep_end_to_end(engine):
    pcm, _, cls = TG.scenario()
    recs = [pcm, pcm[:SHORT].copy()]
    logp = [TG.logp_of(cls), TG.logp_of(scenario_cls(SHORT))]
    refs = [[(a, b, f"voice{v}") for v, a, b in TG.LAYOUT], [(a, min(b, 20.0), f"voice{v}") for v, a, b in TG.LAYOUT if a < 20.0]]
    d = dz.Diarizer(engine, None, sub("resnet").ResNet34(engine, sub("resnet").synthetic_weights(0), precision=0))
    kw = dict(step_s=TG.STEP_S, min_cluster_size=TG.E2E_MIN_CLUSTER, logp=logp)
    singles = []
    for t in THRESHOLDS:
        results = d.run_many(recs, threshold=t, **kw)
        scored = d.score(results, refs)
        for res, one, n, ref in zip(results, scored, (len(pcm), SHORT), refs):
            want = DRF.der_ref(res.speakers, n, ref, K=res.n_speakers)
            assert tallies_of(one) == (want["scored"], want["total"], want["missed"], want["false_alarm"], want["confusion"], want["correct"])
            assert np.array_equal(one.co, want["co"]) and one.der == want["der"] and list(one.mapping) == want["names"]
        singles.append((results, scored))
    sweep = d.sweep(recs, refs, THRESHOLDS, **kw)
    three = [dict(s) for s in d.last_sync]
    for t, (results, scored) in enumerate(singles):
        for r in range(2):
            assert tallies_of(sweep.per_recording[t][r]) == tallies_of(scored[r]), (t, r)
            assert np.array_equal(sweep.per_recording[t][r].co, scored[r].co) and sweep.per_recording[t][r].der == scored[r].der
        assert tallies_of(sweep.pooled[t]) == tallies_of(sc.pool(scored))
        print(f"threshold {THRESHOLDS[t]:.4f}: speakers {[res.n_speakers for res in results]} pooled DER {sweep.pooled[t].der:.4f} "
              f"(missed {sweep.pooled[t].missed} false alarm {sweep.pooled[t].false_alarm} confusion {sweep.pooled[t].confusion} of {sweep.pooled[t].total}); "
              f"per recording {[round(x.der, 4) for x in sweep.per_recording[t]]}")
    assert all(p.total > 0 for p in sweep.pooled)
    assert len({tallies_of(p) for p in sweep.pooled}) > 1                  # the three pooled results are not all equal
    assert [res.n_speakers for res in singles[2][0]] == [1, 1] and sweep.pooled[2].confusion > 0
    assert sweep.thresholds == THRESHOLDS and sweep.best == min(range(3), key=lambda t: (sweep.pooled[t].der, abs(THRESHOLDS[t] - THRESHOLDS[1]), THRESHOLDS[t]))
    one = d.sweep(recs, refs, THRESHOLDS[:1], **kw)
    assert len(three) == len(d.last_sync) == 1 and d.last_sync[0]["downloads"] == three[0]["downloads"]       # the waits do not grow with the thresholds
    assert tallies_of(one.pooled[0]) == tallies_of(sweep.pooled[0])
    print(f"sweep: best threshold {sweep.thresholds[sweep.best]:.4f}; waits per pack {three[0]}")


def test_backend_scores_and_tunes_from_rttm(engine, monkeypatch, tmp_path):
    """Backend.score_diarization and Backend.tune_diarization with the models' own (noise-like) class tables: an RTTM file in, DER out, equal to
    score_host on the downloaded speakers tables; an empty recording rides along."""
    for k in ("SDK_MODEL", "SDK_NO_TORCH", "SDK_PRECISION", "SDK_RESNET_WEIGHTS", "SDK_SEGMENTATION_WEIGHTS", "SDK_DIARIZE_MODEL"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SDK_DIARIZE_BATCH", "5")
    be = sub("backend").Backend()
    pcm, _, _ = TG.scenario()
    recs = [pcm[:23 * RATE + 333], np.zeros(0, np.int16), pcm[20 * RATE:32 * RATE]]
    turns = [[(2.0, 13.0, 0), (15.0, 23.0, 1)], [], [(0.0, 7.0, 1), (4.0, 12.0, 0)]]
    uris = ["a", "b", "c"]
    path = tmp_path / "dev.rttm"
    path.write_text("".join(dz.to_rttm(t, u) for t, u in zip(turns, uris)))
    refs = sc.references_for({**sc.parse_rttm(path.read_text()), "b": []}, uris)
    kw = dict(step_s=1.0, min_cluster_size=2)
    ths = [0.4, 0.6]
    with pytest.raises(ValueError, match="no uri"):
        be.score_diarization(be.diarize_many(recs[1:2]), str(path), uris=["b"])          # the file holds no line for the empty recording
    for t, th in enumerate(ths):
        results = be.diarize_many(recs, threshold=th, **kw)
        got = be.score_diarization(results, refs, collar_s=0.25)
        from_file = be.score_diarization([results[0], results[2]], path, uris=["a", "c"], collar_s=0.25)
        want = [sc.score_host(res.speakers, len(x), ref, 0.25) for res, x, ref in zip(results, recs, refs)]
        assert [tallies_of(g) for g in got] == [tallies_of(w) for w in want] and all(np.array_equal(g.co, w.co) for g, w in zip(got, want))
        assert [tallies_of(g) for g in from_file] == [tallies_of(want[0]), tallies_of(want[2])]
        if t == 0:
            sweep = be.tune_diarization(recs, refs, ths, collar_s=0.25, **kw)
        assert [tallies_of(g) for g in sweep.per_recording[t]] == [tallies_of(w) for w in want]
        print(f"backend threshold {th}: speakers {[r.n_speakers for r in results]} pooled DER {sc.pool(got).der:.4f}")
    assert tallies_of(sweep.per_recording[0][1]) == (0, 0, 0, 0, 0, 0) and sweep.per_recording[0][1].der == 0.0
