"""GPU checks of the smoothing of diarized turns (csrc/smooth.hip, smooth.py): sdk_smooth_turns's table and tallies bit for bit against
smooth.smooth_host on every shared case of tests/smooth_ref.py - the sizes around a workgroup of T = 256 frames, packs whose boundaries lie
inside a workgroup, on its edge and around an empty recording, every fill and keep the issue names, both caps, K_r of 1, 3 and 40, gaps and
runs astride a workgroup's edge - and on seeded random run-structured packs, twice with equal bytes; the refusals; then run, run_many, sweep
and backend.smooth_diarization on the smallest recordings of tests/test_diarize_many_gpu.py with injected class tables.

The kernels stage no halo (a walk reads across the edge of its workgroup from memory), so "the halo length" of the case list is T itself:
the longest walk that ends inside the neighbouring workgroup.  Every case asserts on the host, with the loop reference, that it shows what
it is for before the device is asked."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import smooth_ref as SR
import test_diarize_gpu as TG
import test_diarize_many_gpu as MG
from conftest import sub

sm = sub("smooth")
dz = sub("diarize")
sc = sub("score")
LIB = sub("_lib")
pytestmark = pytest.mark.gpu

CASES = SR.cases()


@functools.lru_cache(maxsize=None)
def case_of(name):
    """(case, the host's table, tallies, crowded frames), made once; the case shows what it is for."""
    c = CASES[name] if isinstance(name, str) else SR.random_pack(name)
    want, tal = sm.smooth_host(c["sp"], c["frame_off"], c["cent_off"], c["fill"], c["keep"], c["cap"])
    ref, ref_tal, crowded = SR.smooth_ref(c["sp"], c["frame_off"], c["cent_off"], c["fill"], c["keep"], c["cap"])
    assert np.array_equal(want, ref) and np.array_equal(tal, ref_tal)
    SR.holds(c, want, tal, crowded)
    return c, want, tal, crowded


def on_device(engine, c, fill=None, keep=None, cap=None):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int32))).to(engine.device)  # noqa: E731
    sp_d = up(c["sp"])
    out, tal = sm.smooth_turns(engine, sp_d, (up(c["frame_off"]), up(c["cent_off"])), c["fill"] if fill is None else fill,
                               c["keep"] if keep is None else keep, c["cap"] if cap is None else cap)
    assert torch.equal(sp_d.cpu(), torch.from_numpy(c["sp"]))                      # the input is not touched
    return out.cpu().numpy(), tal.cpu().numpy()


@pytest.mark.parametrize("name", sorted(CASES))
def test_smooth_turns_bit_for_bit_on_every_case(engine, name):
    c, want, want_tal, _ = case_of(name)
    got, tal = on_device(engine, c)
    assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (name, np.argwhere(got != want)[:4].tolist())
    assert tal.dtype == np.int32 and np.array_equal(tal, want_tal), (name, tal.tolist(), want_tal.tolist())


@pytest.mark.parametrize("seed", [31, 32, 33])
def test_random_packs_bit_for_bit_and_twice_the_same_bytes(engine, seed):
    c, want, want_tal, _ = case_of(seed)
    (a, ta), (b, tb) = on_device(engine, c), on_device(engine, c)
    assert np.array_equal(a, want) and np.array_equal(ta, want_tal), (seed, np.argwhere(a != want)[:4].tolist())
    assert a.tobytes() == b.tobytes() and ta.tobytes() == tb.tobytes()
    for fill, keep, cap in ((0, 0, 2), (SR.T, SR.T + 1, 3 - c["cap"]), (SR.MAX, SR.MAX, c["cap"])):     # the canonical form; the longest walks
        h, ht = sm.smooth_host(c["sp"], c["frame_off"], c["cent_off"], fill, keep, cap)
        g, gt = on_device(engine, c, fill, keep, cap)
        assert np.array_equal(g, h) and np.array_equal(gt, ht), (seed, fill, keep, cap)


def test_the_module_fills_drops_and_meets_a_crowded_frame():
    filled = dropped = crowded = 0
    for name in list(CASES) + [31, 32, 33]:
        _, _, tal, cr = case_of(name)
        filled, dropped, crowded = filled + int(tal[:, 0].sum()), dropped + int(tal[:, 1].sum()), crowded + cr
    assert filled > 0 and dropped > 0 and crowded > 0


def test_refusals_are_exceptions_not_faults(engine):
    dev = engine.device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int32))).to(dev)  # noqa: E731
    sp, offs = up(SR.solo("#.#.#")), (up([0, 5]), up([0, 1]))
    for fill, keep in ((1025, 0), (0, 1025), (-1, 0)):
        with pytest.raises(ValueError, match="frames, 0 .. 1024"):
            sm.smooth_turns(engine, sp, offs, fill, keep, 2)
    with pytest.raises(ValueError, match="1 or 2 speakers per frame"):
        sm.smooth_turns(engine, sp, offs, 1, 1, 3)
    with pytest.raises(ValueError, match="speakers must be a contiguous int32 device tensor"):
        sm.smooth_turns(engine, sp.cpu(), offs, 1, 1, 2)
    with pytest.raises(ValueError, match="cent_off must be a contiguous int32 device tensor"):
        sm.smooth_turns(engine, sp, (offs[0], up([0, 1, 2])), 1, 1, 2)
    # the library refuses on its own, before any launch: nothing is written
    lib = engine.lib
    tal = torch.full((1, 2), -7, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.sdk_smooth_turns_workspace_bytes(5), dtype=torch.uint8, device=dev)
    args = lambda fill, keep, cap, nbytes: (engine.ctx, sp.data_ptr(), offs[0].data_ptr(), offs[1].data_ptr(), 1, 5, fill, keep, cap,  # noqa: E731
                                            tal.data_ptr(), ws.data_ptr(), nbytes, None)
    assert lib.sdk_smooth_turns(*args(1025, 0, 2, ws.numel())) != 0 and b"fill_frames=1025" in lib.sdk_last_error()
    assert lib.sdk_smooth_turns(*args(0, 1025, 2, ws.numel())) != 0 and b"keep_frames=1025" in lib.sdk_last_error()
    assert lib.sdk_smooth_turns(*args(1, 1, 3, ws.numel())) != 0 and b"cap=3" in lib.sdk_last_error()
    torch.cuda.synchronize()
    assert (tal.cpu().numpy() == -7).all() and sp.cpu().numpy().tolist() == SR.solo("#.#.#").tolist()
    rc = lib.sdk_smooth_turns(*args(1, 1, 2, 16))
    assert rc != 0 and b"workspace of 16 bytes" in lib.sdk_last_error()
    with pytest.raises(LIB.SdkError, match="workspace of 16 bytes"):
        LIB.check(rc, "sdk_smooth_turns")
    assert lib.sdk_smooth_turns_workspace_bytes(1 << 30) == 0 and b"fewer than 2^30" in lib.sdk_last_error()
    # no frames at all: the tallies are zeroed and nothing else is read
    out, tal0 = sm.smooth_turns(engine, up(np.zeros((0, 2))), (up([0, 0, 0]), up([0, 2, 2])), 3, 3, 2)
    assert out.shape == (0, 2) and tal0.cpu().numpy().tolist() == [[0, 0], [0, 0]]


# ------------------------------------------------------------------------------------------------ end to end
# The class tables of tests/test_diarize_many_gpu.py's recordings B (23 s) and C (5 s) with two dropouts cut into B's turns (0.1 s and
# 0.06 s: 6 and 3 or 4 frames) - what a segmentation model leaves in the middle of a turn.  OFF = 0.15 s fills both (8 frames); ON = 4 s (238
# frames) keeps B's turns, which are 11 s and 8 s long once filled, and drops C's only turn, 3 s.
LAYOUT_B = [(0, 2.0, 7.0), (0, 7.1, 13.0), (1, 15.0, 18.0), (1, 18.06, 27.0)]
OFF, ON = 0.15, 4.0
THRESHOLDS = [0.2, TG.E2E_THRESHOLD]


def cls_of(n_samples, layout):
    """MG.cls_for with a layout of its own."""
    st = MG.seg.chunk_starts(n_samples, TG.STEP_S)
    cls = np.zeros((len(st), MG.F), np.uint8)
    for c in range(len(st)):
        local = {}
        for i in range(MG.F):
            t = (int(st[c]) + 270 * i + 495) / MG.RATE
            on = sorted({v for v, a, b in layout if a <= t < b and t < n_samples / MG.RATE})
            for v in on:
                local.setdefault(v, len(local))
            ids = sorted({local[v] for v in on})
            cls[c, i] = 0 if not ids else ids[0] + 1 if len(ids) == 1 else {(0, 1): 4, (0, 2): 5, (1, 2): 6}[tuple(ids)]
    return cls


@pytest.fixture(scope="module")
def diarized(engine):
    """The recordings, their injected tables, the Diarizer, the default run_many and the smoothed one with their last_sync: made once."""
    pcm, _, _ = TG.scenario()
    recs = [pcm[:MG.N_B].copy(), np.zeros(0, np.int16), pcm[:MG.N_C].copy()]
    logp = [TG.logp_of(cls_of(MG.N_B, LAYOUT_B)), None, TG.logp_of(cls_of(MG.N_C, TG.LAYOUT))]
    d = dz.Diarizer(engine, None, MG.rn.ResNet34(engine, MG.rn.synthetic_weights(0), precision=0))
    kw = dict(step_s=TG.STEP_S, threshold=TG.E2E_THRESHOLD, min_cluster_size=TG.E2E_MIN_CLUSTER, constrained=True)
    plain = d.run_many(recs, logp=logp, **kw)
    sync_plain = [dict(s) for s in d.last_sync]
    smooth = d.run_many(recs, logp=logp, min_duration_off=OFF, min_duration_on=ON, **kw)
    sync_smooth = [dict(s) for s in d.last_sync]
    return d, recs, logp, kw, plain, sync_plain, smooth, sync_smooth


def host_smoothing(res, fill, keep, cap=2):
    out, tal = sm.smooth_host(res.speakers, [0, len(res.speakers)], [0, res.n_speakers], fill, keep, cap)
    return out, tal[0].tolist()


def test_run_many_smooths_on_the_device_without_a_further_wait(engine, diarized):
    d, recs, logp, kw, plain, sync_plain, smooth, sync_smooth = diarized
    fill, keep = sm.fill_frames_of(OFF), sm.keep_frames_of(ON)
    assert (fill, keep) == (8, 238) and sync_smooth == sync_plain
    print(f"run_many: waits per pack {sync_smooth}; smoothing {[r.smoothing for r in smooth]}")
    for r, (a, b) in enumerate(zip(plain, smooth)):
        assert a.smoothing is None
        want, tal = host_smoothing(a, fill, keep)
        assert np.array_equal(b.speakers, want) and b.speakers.dtype == np.int32
        assert b.smoothing == {"min_duration_off": OFF, "min_duration_on": ON, "fill": fill, "keep": keep, "filled": tal[0], "dropped": tal[1]}
        assert b.turns == dz.turns_from_frames(want, a.n_speakers)
        assert np.array_equal(b.labels, a.labels) and np.array_equal(b.count, a.count) and np.array_equal(b.centroids, a.centroids)
        assert b.n_speakers == a.n_speakers and np.array_equal(b.scores, a.scores)
    # the injected dropouts are filled, B's turns stay, C's only turn is shorter than 4 s and goes; the empty recording rides along
    assert smooth[0].smoothing["filled"] > 0 and len(smooth[0].turns) < len(plain[0].turns) and len(smooth[0].turns) >= 2
    assert smooth[2].smoothing["dropped"] > 0 and smooth[2].turns == [] and plain[2].turns and smooth[2].n_speakers == plain[2].n_speakers
    assert smooth[1].turns == [] and smooth[1].smoothing["filled"] == 0
    # only one of the two, and the cap per frame
    only_off = d.run_many(recs, logp=logp, min_duration_off=OFF, **kw)
    assert np.array_equal(only_off[0].speakers, host_smoothing(plain[0], fill, 0)[0]) and only_off[2].turns == plain[2].turns
    one = d.run_many(recs, logp=logp, max_speakers=1, **kw)
    one_s = d.run_many(recs, logp=logp, max_speakers=1, min_duration_off=OFF, min_duration_on=ON, **kw)
    assert np.array_equal(one_s[0].speakers, host_smoothing(one[0], fill, keep, cap=1)[0]) and (one_s[0].speakers[:, 1] == -1).all()
    with pytest.raises(ValueError, match="min_duration_off"):
        d.run_many(recs, logp=logp, min_duration_off=-1.0, **kw)
    with pytest.raises(ValueError, match="min_duration_on"):
        d.run_many(recs, logp=logp, min_duration_on=18.0, **kw)


def test_run_equals_run_many(engine, diarized):
    d, recs, logp, kw, plain, _, smooth, _ = diarized
    for r in (0, 2):
        alone = d.run(recs[r], logp=logp[r], min_duration_off=OFF, min_duration_on=ON, **kw)
        assert np.array_equal(alone.speakers, smooth[r].speakers) and alone.turns == smooth[r].turns and alone.smoothing == smooth[r].smoothing
        assert np.array_equal(alone.count, smooth[r].count) and np.array_equal(alone.labels, smooth[r].labels)
    assert d.run(recs[0], logp=logp[0], **kw).smoothing is None
    assert d.run(recs[1], min_duration_off=OFF).smoothing["filled"] == 0


def tallies_of(r):
    return (r.scored, r.total, r.missed, r.false_alarm, r.confusion, r.correct)


def test_sweep_scores_every_pair_in_the_same_download(engine, diarized):
    d, recs, logp, kw, _, _, _, _ = diarized
    refs = [[(a, min(b, MG.N_B / MG.RATE), f"voice{v}") for v, a, b in TG.LAYOUT if a < MG.N_B / MG.RATE], [],
            [(a, min(b, 5.0), f"voice{v}") for v, a, b in TG.LAYOUT if a < 5.0]]
    skw = {k: v for k, v in kw.items() if k != "threshold"}
    plain = d.sweep(recs, refs, THRESHOLDS, logp=logp, **skw)
    sync_plain = [dict(s) for s in d.last_sync]
    both = d.sweep(recs, refs, THRESHOLDS, logp=logp, smoothing=[(0, 0), (OFF, ON)], **skw)
    assert [dict(s) for s in d.last_sync] == sync_plain
    assert isinstance(plain, sc.SweepResult) and isinstance(both, sc.SmoothSweepResult)
    assert both.thresholds == THRESHOLDS and both.smoothing == [(0.0, 0.0), (OFF, ON)]
    fill, keep = sm.fill_frames_of(OFF), sm.keep_frames_of(ON)
    for t, th in enumerate(THRESHOLDS):
        results = d.run_many(recs, logp=logp, **{**kw, "threshold": th})
        for r in range(3):
            assert tallies_of(both.per_recording[t][0][r]) == tallies_of(plain.per_recording[t][r]), (t, r)
            assert np.array_equal(both.per_recording[t][0][r].co, plain.per_recording[t][r].co)
            want = sc.score_host(host_smoothing(results[r], fill, keep)[0], len(recs[r]), refs[r])
            got = both.per_recording[t][1][r]
            assert tallies_of(got) == tallies_of(want) and got.der == want.der, (t, r, tallies_of(got), tallies_of(want))
            assert got.co.shape == (want.co.shape[0], results[r].n_speakers) and np.array_equal(got.co[:, :want.co.shape[1]], want.co)
        assert [tallies_of(p) for p in both.pooled[t]] == [tallies_of(sc.pool(row)) for row in both.per_recording[t]]
    flat = [(both.pooled[t][s].der, abs(th - dz.PYANNOTE_THRESHOLD), th, s) for t, th in enumerate(THRESHOLDS) for s in range(2)]
    _, _, th, s = min(flat)
    assert both.best == (th, *both.smoothing[s])
    print(f"sweep: pooled DER {[[round(p.der, 4) for p in row] for row in both.pooled]}, best {both.best}, waits per pack {sync_plain}")
    with pytest.raises(ValueError, match="smoothing="):
        d.sweep(recs, refs, THRESHOLDS, logp=logp, smoothing=[], **skw)


def test_smooth_diarization_on_finished_results(engine, diarized, monkeypatch):
    d, recs, logp, kw, plain, _, smooth, _ = diarized
    bk = sub("backend")
    be = bk.Backend()
    monkeypatch.setattr(be, "engine", lambda: engine)
    got = bk.smooth_diarization(be, plain, OFF, ON)
    assert len(got) == 3
    for a, b, c in zip(plain, smooth, got):
        assert c is not a and np.array_equal(c.speakers, b.speakers) and c.turns == b.turns and c.smoothing == b.smoothing
        assert a.smoothing is None and c.count is a.count and c.n_speakers == a.n_speakers
    single = bk.smooth_diarization(be, plain[0], min_duration_off=OFF)
    assert np.array_equal(single.speakers, host_smoothing(plain[0], sm.fill_frames_of(OFF), 0)[0])
    capped = bk.smooth_diarization(be, plain, OFF, ON, max_speakers=1)
    assert np.array_equal(capped[0].speakers, host_smoothing(plain[0], sm.fill_frames_of(OFF), sm.keep_frames_of(ON), cap=1)[0])
    assert bk.smooth_diarization(be, []) == []
