"""GPU checks of scoring the DIHARD way (csrc/score_jer.hip, score.py): sdk_score_uem, sdk_score_durations, sdk_score_jaccard and sdk_score_map on
the Jaccard table, bit for bit against the numpy restatements of score.py on a pack that crosses every edge of the kernels' walks, then the
public calls with and without the new keywords.  Every comparison is integer equality."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import der_ref as DRF
import test_der_gpu as TD
import test_diarize_gpu as TG
from conftest import sub

sc = sub("score")
dz = sub("diarize")
LIB = sub("_lib")
pytestmark = pytest.mark.gpu

HOP, FIRST, RATE = 270, 495, 16000
ONE = 1 << 30
# Frames per recording.  The packed grid: 0 | 0 .. 2 | 3 .. 702 | 703 .. 4815 | 4816 .. 5116 | 5117 .. 6016.  The durations kernel's workgroups
# take 4096 frames: the first serves recordings 1, 2 and the head of 3, the second the tail of 3 (4096 + 17 frames: it straddles), 4 and 5.
G_R = [0, 3, 700, 4096 + 17, 301, 900]
S_R = [2, 1, 3, 4, 3, 64]
K_R = [1, 2, 3, 4, 2, 64]
N_SAMPLES = [HOP * g + 226 if g else 0 for g in G_R]             # global_frames(n) == g


def centre_s(g: int, plus: int = 0) -> float:
    t = (HOP * g + FIRST + plus) / RATE
    assert sc.to_samples(t) == HOP * g + FIRST + plus
    return t


# [] on the 3-frame recording; one region from a centre (in) to one sample past a centre (in); None; three regions - one holding no centre, one
# from one sample past a centre (out) to a centre (out), one across the workgroup boundary; a region running past the end; None at 64 x 64
UEMS = [[(0.0, 1.0)], [], [(centre_s(100), centre_s(600, 1))], [(centre_s(2000, 1), centre_s(2001)), (centre_s(10, 1), centre_s(1500)), (centre_s(3000), centre_s(4100))],
        [(centre_s(150), 1000.0)], None]


def tables(engine, K_r=K_R):
    tab = dz.GroupTables(engine, np.zeros(len(G_R) + 1, np.int64), np.concatenate([[0], np.cumsum(G_R)]), N_SAMPLES)
    return tab.set_clusters(np.concatenate([[0], np.cumsum(K_r)]))


@functools.lru_cache(maxsize=None)
def pack_case():
    rng = np.random.default_rng(3600)
    refs = [DRF.random_turns(rng, S, n) for S, n in zip(S_R, N_SAMPLES)]
    hyps = [DRF.random_speakers(rng, G, K) for G, K in zip(G_R, K_R)]
    for r, K in ((2, 3), (3, 4), (5, 64)):                      # a speaker named twice, names >= K_r (alone and beside a real one), nobody
        for g0 in (5, 120, G_R[r] - 9):
            hyps[r][g0:g0 + 4] = [[1, 1], [K, -1], [0, K + 5], [-1, -1]]
    return refs, hyps


@functools.lru_cache(maxsize=None)
def restated(collar_s: float, skip: bool, with_uem: bool = True):
    """The host restatement per recording, with the K_r of the tables (a name >= K_r counts for nobody)."""
    refs, hyps = pack_case()
    out = []
    for r, (G, S, K) in enumerate(zip(G_R, S_R, K_R)):
        merged, names = sc.prepare_reference(refs[r])
        assert len(names) == S
        mask, scored = sc.reference_masks_host(merged, G, sc.collar_samples(collar_s), skip)
        if with_uem:
            scored = scored & sc.uem_mask_host(sc.prepare_uem(UEMS[r]), G)
        co, tally = sc.cooccur_host(mask, scored, hyps[r], S, K)
        rf, hf = sc.durations_host(mask, scored, hyps[r], S, K)
        q = sc.jaccard_table_host(co, rf, hf)
        jmap, jsum = sc.assignment_host(q)
        out.append(dict(names=names, scored=scored, co=co, tally=tally, ref_frames=rf, hyp_frames=hf, q=q, jsum=jsum, correct=sc.assignment_host(co)[1]))
    return out


def up(engine, a, t):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(t))).to(engine.device)


def jaccard_dev(engine, co, rf, hf, ref_off, cent_off, co_off):
    """sdk_score_jaccard, then sdk_score_map on its table, on device tensors -> (q, map, jsum) as numpy."""
    R, total = len(ref_off) - 1, int(co_off[-1])
    ref_d, cent_d, off_d = up(engine, ref_off, np.int32), up(engine, cent_off, np.int32), up(engine, co_off, np.int64)
    q = torch.full((max(total, 1),), -7, dtype=torch.int32, device=engine.device)
    mapping = torch.full((max(int(ref_off[-1]), 1),), -7, dtype=torch.int32, device=engine.device)
    jsum = torch.full((R,), -7, dtype=torch.int64, device=engine.device)
    LIB.check(engine.lib.sdk_score_jaccard(engine.ctx, co.data_ptr(), rf.data_ptr(), hf.data_ptr(), ref_d.data_ptr(), cent_d.data_ptr(), off_d.data_ptr(), R, total,
                                           q.data_ptr(), None), "sdk_score_jaccard")
    S_max, K_max = int(np.diff(ref_off).max()), int(np.diff(cent_off).max())
    LIB.check(engine.lib.sdk_score_map(engine.ctx, q.data_ptr(), ref_d.data_ptr(), cent_d.data_ptr(), off_d.data_ptr(), R, S_max, K_max, mapping.data_ptr(),
                                       jsum.data_ptr(), None), "sdk_score_map")
    return q.cpu().numpy()[:total], mapping.cpu().numpy()[:int(ref_off[-1])], jsum.cpu().numpy()


def check_map(m, table, value):
    used = m[m >= 0]
    assert ((m >= -1) & (m < table.shape[1])).all() and len(set(used.tolist())) == len(used)
    assert all(table[i, j] > 0 for i, j in enumerate(m) if j >= 0) and sum(int(table[i, j]) for i, j in enumerate(m) if j >= 0) == int(value)


@pytest.mark.parametrize("collar_s,skip", [(0.0, False), (0.25, True)])
def test_uem_durations_jaccard_and_map_bit_for_bit(engine, collar_s, skip):
    refs, hyps = pack_case()
    want = restated(collar_s, skip)
    assert sum(w["scored"].sum() for w in want) > 0 and any(w["scored"].sum() < G for w, G in zip(want, G_R))
    tab = tables(engine)
    spk = torch.from_numpy(np.concatenate(hyps)).to(engine.device)
    ref = sc.rasterise_references(engine, tab, refs, collar_s, skip, uems=UEMS)
    scored = ref.scored.cpu().numpy()
    assert scored.shape == (tab.G,)
    st = sc.score_tables(engine, spk, tab, ref, jer=True)
    co_off = st.co_off
    q, q_map, q_sum = jaccard_dev(engine, st.co, st.ref_frames, st.hyp_frames, ref.ref_off, tab.cent_off, co_off)
    tally, correct, co, rf, hf, jsum, jmap = (t.cpu().numpy() for t in (st.tally, st.correct, st.co, st.ref_frames, st.hyp_frames, st.jsum, st.jer_mapping))
    assert rf.shape == (sum(S_R),) and hf.shape == (sum(K_R),) and rf.dtype == hf.dtype == q.dtype == np.int32
    assert np.array_equal(q_sum, jsum) and np.array_equal(q_map, jmap)                      # the test's own launches: the same bytes
    for r, w in enumerate(want):
        g0, g1, i0, i1, j0, j1, a = (int(v) for v in (tab.frame_off[r], tab.frame_off[r + 1], ref.ref_off[r], ref.ref_off[r + 1], tab.cent_off[r],
                                                         tab.cent_off[r + 1], co_off[r]))
        assert np.array_equal(scored[g0:g1], w["scored"]), r
        assert np.array_equal(co[a:a + S_R[r] * K_R[r]].reshape(S_R[r], K_R[r]), w["co"]) and np.array_equal(tally[r], w["tally"]), r
        assert np.array_equal(rf[i0:i1], w["ref_frames"]) and np.array_equal(hf[j0:j1], w["hyp_frames"]), r
        assert np.array_equal(q[a:a + S_R[r] * K_R[r]].reshape(S_R[r], K_R[r]), w["q"]), r
        assert int(jsum[r]) == w["jsum"] and int(correct[r]) == w["correct"], r
        check_map(jmap[i0:i1], w["q"], jsum[r])
    print(f"collar {collar_s} skip {skip}: scored {[int(w['scored'].sum()) for w in want]} of {G_R}, jsum / 2^30 {[round(w['jsum'] / ONE, 3) for w in want]}")


def test_uem_alone_keeps_what_the_reference_left(engine):
    """sdk_score_uem only clears: a frame the collar removed stays removed; with no interval at all nothing is scored."""
    refs, _ = pack_case()
    tab = tables(engine)
    plain = sc.rasterise_references(engine, tab, refs, 0.25, True).scored.cpu().numpy()
    none = sc.rasterise_references(engine, tab, refs, 0.25, True, uems=[None] * len(G_R)).scored.cpu().numpy()
    assert np.array_equal(none, plain) and 0 < plain.sum() < tab.G
    nothing = sc.rasterise_references(engine, tab, refs, 0.25, True, uems=[[]] * len(G_R)).scored.cpu().numpy()
    assert not nothing.any()
    with_uem = sc.rasterise_references(engine, tab, refs, 0.25, True, uems=UEMS).scored.cpu().numpy()
    assert not (with_uem & ~plain.astype(bool)).any() and with_uem.sum() == sum(int(w["scored"].sum()) for w in restated(0.25, True))
    lib = engine.lib
    buf = torch.ones((8,), dtype=torch.uint8, device=engine.device)
    assert lib.sdk_score_uem(engine.ctx, None, None, None, 0, 0, 8, buf.data_ptr(), None) != 0 and b"R at least 1" in lib.sdk_last_error()
    z = torch.zeros((4,), dtype=torch.int32, device=engine.device)
    assert lib.sdk_score_durations(engine.ctx, None, None, None, z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, 0, 65, 1, z.data_ptr(), z.data_ptr(), None) != 0
    assert b"at most 64" in lib.sdk_last_error()
    assert lib.sdk_score_durations(engine.ctx, None, None, None, z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, 0, 1, 65, z.data_ptr(), z.data_ptr(), None) != 0
    assert b"at most 64" in lib.sdk_last_error()
    assert buf.cpu().numpy().all()                                         # a refusal comes before any launch


def test_jaccard_on_hand_made_tables(engine):
    big = (1 << 31) - 1
    equal = (np.full((4, 4), 50), np.full(4, 200), np.full(4, 200))        # every pair 50 / 350: the map is free, jsum is not
    cases = [(np.array([[1]]), np.array([big]), np.array([big])), (np.array([[big]]), np.array([big]), np.array([big])), equal,
             (np.zeros((3, 0), np.int64), np.array([5, 0, 7]), np.zeros(0, np.int64)),                     # K_r = 0
             (np.array([[big // 2, 0], [0, 7]]), np.array([big, 9]), np.array([big, 7]))]
    ref_off = np.concatenate([[0], np.cumsum([c[0].shape[0] for c in cases])])
    cent_off = np.concatenate([[0], np.cumsum([c[0].shape[1] for c in cases])])
    co_off = np.concatenate([[0], np.cumsum([c[0].size for c in cases])]).astype(np.int64)
    co, rf, hf = (up(engine, np.concatenate([c[k].reshape(-1) for c in cases]), np.int32) for k in range(3))
    q, mapping, jsum = jaccard_dev(engine, co, rf, hf, ref_off, cent_off, co_off)
    want = [sc.jaccard_table_host(*c) for c in cases]
    assert np.array_equal(q, np.concatenate([w.reshape(-1) for w in want]))
    assert q[0] == 0 and q[1] == ONE and (q[2:18] == (50 * ONE) // 350).all() and q[18] == ((big // 2) << 30) // (2 * big - big // 2) and q[21] == (7 * ONE) // 9
    assert jsum.tolist() == [0, ONE, 4 * ((50 * ONE) // 350), 0, int(q[18]) + int(q[21])]
    assert mapping[0] == -1 and mapping[1] == 0 and sorted(mapping[2:6].tolist()) == [0, 1, 2, 3] and mapping[6:9].tolist() == [-1, -1, -1]
    for r, w in enumerate(want):
        assert int(jsum[r]) == sc.assignment_host(w)[1]
    assert engine.lib.sdk_score_jaccard(engine.ctx, co.data_ptr(), rf.data_ptr(), hf.data_ptr(), None, None, None, 1, 64 * 64 + 1, co.data_ptr(), None) != 0


# ------------------------------------------------------------------------------------------------ the public calls
def tallies_of(r):
    return (r.scored, r.total, r.missed, r.false_alarm, r.confusion, r.correct)


def jer_of(r):
    return (r.jsum, r.ref_speakers, r.jer, r.purity, r.coverage, r.pc_sums, r.jer_mapping, r.ref_frames.tolist(), r.hyp_frames.tolist())


def same_result(got, want):
    assert tallies_of(got) == tallies_of(want) and got.der == want.der and np.array_equal(got.co, want.co) and list(got.mapping) == list(want.mapping)
    if want.jer is None:
        assert all(getattr(got, f) is None for f in ("jer", "jsum", "ref_speakers", "ref_frames", "hyp_frames", "jer_mapping", "purity", "coverage"))
        return
    assert jer_of(got)[:6] == jer_of(want)[:6] and jer_of(got)[7:] == jer_of(want)[7:]
    q = sc.jaccard_table_host(got.co, got.ref_frames, got.hyp_frames)
    check_map(np.array([got.jer_mapping[nm] for nm in want.mapping], np.int64), q, got.jsum)


def public_case():
    """Speakers tables whose names stay below K_r, as a DiarizationResult's do, and the results that carry them."""
    refs, _ = pack_case()
    rng = np.random.default_rng(3603)
    hyps = [DRF.random_speakers(rng, G, K) for G, K in zip(G_R, K_R)]
    results = [dz.DiarizationResult([], K, np.zeros((K, 4), np.float32), np.zeros((0, 3), np.int32), (h >= 0).sum(1).astype(np.uint8), h, np.zeros(0, np.int64),
                                    np.zeros((0, 3, 4), np.int32)) for h, K in zip(hyps, K_R)]
    return refs, hyps, results


def test_score_grouped_and_diarizer_score_with_uem_and_jer(engine):
    refs, hyps, results = public_case()
    d = dz.Diarizer(engine, None, None)
    spk = torch.from_numpy(np.concatenate(hyps)).to(engine.device)
    for collar_s, skip in ((0.0, False), (0.25, True)):
        want = [sc.score_host(h, n, t, collar_s, skip, uem=u, jer=True) for h, n, t, u in zip(hyps, N_SAMPLES, refs, UEMS)]
        # score_host takes K from the names it sees; these tables name every speaker but perhaps the last of a few
        grouped = sc.score_grouped(engine, spk, tables(engine, [len(w.hyp_frames) for w in want]), refs, collar_s, skip, uems=UEMS, jer=True)
        scored = d.score(results, refs, collar_s, skip, uem=UEMS, jer=True)
        again = d.score(results, refs, collar_s, skip, uem=UEMS, jer=True)
        for r, (g, s, a, w) in enumerate(zip(grouped, scored, again, want)):
            same_result(g, w)
            assert tallies_of(s) == tallies_of(w) and s.der == w.der and s.jsum == w.jsum and s.ref_speakers == w.ref_speakers and s.jer == w.jer, r
            assert s.ref_frames.tolist() == w.ref_frames.tolist() and s.hyp_frames[:len(w.hyp_frames)].tolist() == w.hyp_frames.tolist() and not s.hyp_frames[len(w.hyp_frames):].any()
            assert (s.purity, s.coverage) == (w.purity, w.coverage)
            assert jer_of(a) == jer_of(s) and a.co.tobytes() == s.co.tobytes() and a.ref_frames.tobytes() == s.ref_frames.tobytes() and a.mapping == s.mapping
        pooled = sc.pool(scored)
        assert (pooled.jsum, pooled.ref_speakers, pooled.jer, pooled.purity, pooled.coverage) == tuple(getattr(sc.pool(want), f) for f in ("jsum", "ref_speakers", "jer", "purity", "coverage"))
        print(f"collar {collar_s} skip {skip}: pooled DER {pooled.der:.4f} JER {pooled.jer:.4f} purity {pooled.purity:.4f} coverage {pooled.coverage:.4f}")
    # a UEM file read with uris: recording "r3" is not in it and is scored everywhere
    text = "".join(f"r{r} 1 {a:.6f} {b:.6f}\n" for r, u in enumerate(UEMS) if u is not None for a, b in u)
    from_file = d.score(results, refs, uem=text, uris=[f"r{r}" if r != 1 else "absent" for r in range(len(G_R))], jer=True)
    assert from_file[1].scored == G_R[1] and from_file[2].scored == 501 and from_file[5].scored == G_R[5]


def test_defaults_run_the_untouched_path(engine):
    refs, hyps, results = public_case()
    tab = tables(engine)
    spk = torch.from_numpy(np.concatenate(hyps)).to(engine.device)
    ref = sc.rasterise_references(engine, tab, refs, 0.25, False)
    st = sc.score_tables(engine, spk, tab, ref)
    flat = torch.cat([st.tally.reshape(-1), st.correct, st.mapping.to(torch.int64), st.co.to(torch.int64)]).cpu().numpy()
    assert flat.shape == (st.size,) and all(getattr(st, f) is None for f in ("ref_frames", "hyp_frames", "jsum", "jer_mapping"))
    want = st.results(ref, flat)
    host = [sc.score_host(h, n, t, 0.25, False) for h, n, t in zip(hyps, N_SAMPLES, refs)]
    d = dz.Diarizer(engine, None, None)
    for got in (sc.score_grouped(engine, spk, tab, refs, 0.25, False), sc.score_grouped(engine, spk, tab, refs, 0.25, False, uems=None, jer=False),
                d.score(results, refs, 0.25), d.score(results, refs, 0.25, uem=None, jer=False)):
        for g, w, h in zip(got, want, host):
            same_result(g, w)
            assert g.mapping == w.mapping and tallies_of(g) == tallies_of(h)
    only_uem = d.score(results, refs, 0.25, uem=UEMS)                      # the map without the Jaccard part: a DER, the new fields None
    for g, u, h, n, t in zip(only_uem, UEMS, hyps, N_SAMPLES, refs):
        assert tallies_of(g) == tallies_of(sc.score_host(h, n, t, 0.25, False, uem=u)) and g.jer is None and g.ref_frames is None


def test_sweep_with_uem_and_jer(engine):
    pcm, _, cls = TG.scenario()
    recs = [pcm, pcm[:TD.SHORT].copy()]
    logp = [TG.logp_of(cls), TG.logp_of(TD.scenario_cls(TD.SHORT))]
    refs = [[(a, b, f"voice{v}") for v, a, b in TG.LAYOUT], [(a, min(b, 20.0), f"voice{v}") for v, a, b in TG.LAYOUT if a < 20.0]]
    uems = [[(3.0, 17.5), (17.5, 30.0), (35.0, 100.0)], None]
    d = dz.Diarizer(engine, None, sub("resnet").ResNet34(engine, sub("resnet").synthetic_weights(0), precision=0))
    kw = dict(step_s=TG.STEP_S, min_cluster_size=TG.E2E_MIN_CLUSTER, logp=logp)
    plain = d.sweep(recs, refs, TD.THRESHOLDS, **kw)
    waits = [dict(s) for s in d.last_sync]
    sweep = d.sweep(recs, refs, TD.THRESHOLDS, metric="jer", jer=True, uem=uems, **kw)
    assert [dict(s) for s in d.last_sync] == waits and len(waits) == 1     # no more uploads or downloads per pack
    for t, th in enumerate(TD.THRESHOLDS):
        results = d.run_many(recs, threshold=th, **kw)
        for r, (res, x) in enumerate(zip(results, recs)):
            want = sc.score_host(res.speakers, len(x), refs[r], uem=uems[r], jer=True)
            got = sweep.per_recording[t][r]
            assert tallies_of(got) == tallies_of(want) and got.der == want.der, (t, r)
            assert (got.jsum, got.ref_speakers, got.jer) == (want.jsum, want.ref_speakers, want.jer), (t, r)
            assert got.ref_frames.tolist() == want.ref_frames.tolist() and got.hyp_frames[:len(want.hyp_frames)].tolist() == want.hyp_frames.tolist()
            assert (got.purity, got.coverage) == (want.purity, want.coverage)
            same = sc.score_host(res.speakers, len(x), refs[r])
            assert tallies_of(plain.per_recording[t][r]) == tallies_of(same) and plain.per_recording[t][r].jer is None
        pooled = sc.pool(sweep.per_recording[t])
        assert (sweep.pooled[t].jsum, sweep.pooled[t].ref_speakers, sweep.pooled[t].jer) == (pooled.jsum, pooled.ref_speakers, pooled.jer)
        print(f"threshold {th:.4f}: pooled DER {sweep.pooled[t].der:.4f} JER {sweep.pooled[t].jer:.4f} (S' {sweep.pooled[t].ref_speakers})")
    mid = TD.THRESHOLDS[1]
    assert sweep.best == min(range(3), key=lambda t: (sweep.pooled[t].jer, abs(TD.THRESHOLDS[t] - mid), TD.THRESHOLDS[t]))
    assert plain.best == min(range(3), key=lambda t: (plain.pooled[t].der, abs(TD.THRESHOLDS[t] - mid), TD.THRESHOLDS[t]))
    assert all(p.ref_speakers > 0 for p in sweep.pooled) and len({p.jsum for p in sweep.pooled}) > 1
