"""GPU checks of the fusion of several diarizations (csrc/fuse.hip, fuse.py): every launch against the loop-per-frame restatement of
tests/fuse_ref.py, exact integer equality, with every output tensor pre-filled with a poison pattern so that an element nobody wrote
shows.  The pack: R = 6 recordings of 0, 1, B - 1, B, B + 1 and 3 B + 7 frames (B = fuse.FUSE_BLOCK_FRAMES: a workgroup starts, ends and
crosses recordings, and one recording is empty), H in {2, 3, 8}, K mixed from {0, 1, 2, 5, 64}, masks of 0 to 4 bits a frame with stray bits
at or above K.  Then the hand-worked label cases of tests/test_fuse_cpu.py, the public calls end to end from results and turn lists mixed,
twice with equal bytes, and the single-fault refusals of every tensor of every wrapper."""
from __future__ import annotations

import copy
import functools

import numpy as np
import pytest
import torch

import fuse_ref as FR
import test_fuse_cpu as TC
import test_ops_args_gpu as OA
from conftest import sub

fu = sub("fuse")
sc = sub("score")
LIB = sub("_lib")
pytestmark = pytest.mark.gpu

POISON = {torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A, torch.uint8: 0x5A}


@pytest.fixture
def poisoned(monkeypatch):
    """While it holds, every tensor torch.empty makes is filled with a poison pattern: what a wrapper allocates and no kernel writes shows."""
    real = torch.empty

    def empty(*a, **k):
        t = real(*a, **k)
        return t.fill_(POISON[t.dtype]) if t.dtype in POISON else t
    monkeypatch.setattr(torch, "empty", empty)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_masks(masks):
    return dev(np.ascontiguousarray(masks, dtype=np.uint64).view(np.int64))


@functools.lru_cache(maxsize=None)
def edge_pack(H):
    """(masks, frame_off, K, the restatement's tables under the rank weights at cap 2), made once."""
    masks, off, K = FR.random_pack(100 + H, H, FR.EDGE_FRAMES)
    assert set(K.reshape(-1).tolist()) <= {0, 1, 2, 5, 64}
    return masks, off, K, FR.fuse_ref(masks.tolist(), off, K.tolist())


def host(t):
    return t.cpu().numpy()


def test_masks_from_speakers_tables(engine, poisoned):
    rng = np.random.default_rng(5)
    G_r, K_r = [FR.B + 3, 2, 0, 2 * FR.B - 1], [64, 1, 5, 0]
    off = np.concatenate([[0], np.cumsum(G_r)])
    sp = rng.integers(-2, 66, (int(off[-1]), 2)).astype(np.int32)
    sp[:4] = [[-1, 63], [63, 63], [64, 0], [0, -1]]                              # -1, doubled, at K, and the top bit
    sp[FR.B + 3:FR.B + 5] = [[0, 0], [1, 0]]                                     # K = 1: doubled, and a name at K
    for h, Kh in enumerate([K_r, K_r[::-1]]):
        tab = fu.FuseTables([K_r, K_r[::-1]], off).to(engine)
        got = host(fu.fuse_masks(engine, dev(sp), tab, h)).view(np.uint64)
        want = np.concatenate([np.asarray(FR.masks_ref(sp[off[r]:off[r + 1]], Kh[r]), dtype=np.uint64) for r in range(4)])
        assert np.array_equal(got, want), (h, np.argwhere(got != want)[:4].tolist())
        assert got[:4].tolist() == ([1 << 63, 1 << 63, 1, 1] if h == 0 else [0, 0, 0, 0]) and got[FR.B + 3:FR.B + 5].tolist() == ([1, 1] if h == 0 else [1, 3])
        assert np.array_equal(want, np.concatenate([fu.masks_host(sp[off[r]:off[r + 1]], Kh[r]) for r in range(4)]))


@pytest.mark.parametrize("H", [2, 3, 8])
def test_cooccur_labels_and_vote_on_the_edge_pack(engine, poisoned, H):
    masks, off, K, want = edge_pack(H)
    tab = fu.FuseTables(K, off).to(engine)
    m_d = dev_masks(masks)
    co, tally = fu.fuse_cooccur(engine, m_d, tab)
    assert co.dtype == torch.int32 and tally.dtype == torch.int64
    assert np.array_equal(host(co), want["co"]) and np.array_equal(host(tally), want["tally"]), H
    mapping, correct = fu.pair_map(engine, co, tab)
    assert np.array_equal(host(correct), want["correct"])
    for weights, cap in ((None, 2), (list(range(9, 9 + H)), 1), (None, 1), ([65536] * H, 2)):
        ref = want if (weights is None and cap == 2) else FR.fuse_ref(masks.tolist(), off, K.tolist(), weights, cap)
        w_d = None if weights is None else dev(np.asarray(weights, np.int32))
        dis, order, weight, label_of, n_labels, overflow = fu.fuse_labels(engine, co, tally, correct, tab, w_d)
        got = {"dis": dis, "order": order, "weight": weight, "label_of": label_of, "n_labels": n_labels, "overflow": overflow}
        got["speakers"], got["tallies"] = fu.fuse_vote(engine, m_d, label_of, weight, overflow, tab, cap)
        assert got["speakers"].dtype == torch.int32 and got["tallies"].dtype == torch.int64 and dis.dtype == torch.int64
        got = {k: host(v) for k, v in got.items()}
        assert FR.same(got, ref, list(got)) is None, (H, weights, cap, FR.same(got, ref, list(got)))
    assert want["tallies"][:, 0].sum() > 0 and (want["tallies"][:, 2] < np.diff(off)).any()      # somebody is named, and not every frame is unanimous


@pytest.mark.parametrize("case", ["greedy_tie", "transpose", "overflow"])
@pytest.mark.parametrize("weights", [None, "given"])
def test_labels_on_the_hand_worked_cases(engine, poisoned, case, weights):
    masks, off, K = getattr(FR, "case_" + case)()
    w = None if weights is None else list(range(4, 4 + len(K)))
    want = FR.fuse_ref(masks.tolist(), off, K.tolist(), w)
    tab = fu.FuseTables(K, off).to(engine)
    got = {k: host(v) for k, v in fu.fuse_tables(engine, dev_masks(masks), tab, None if w is None else dev(np.asarray(w, np.int32))).items()}
    assert FR.same(got, want) is None, (case, FR.same(got, want))
    if case == "overflow":
        assert got["n_labels"].tolist() == [64] and got["overflow"].tolist() == [56] and got["tallies"][0, 3] == 56
    if case == "transpose" and w is None:
        assert got["order"].tolist() == [[2, 1, 0]]


@pytest.mark.parametrize("seed,H,frames", [(11, 4, [FR.B, 40]), (12, 7, [300]), (13, 8, [5, 0, 0, 2 * FR.B + 1])])
def test_random_packs_twice_with_the_same_bytes(engine, poisoned, seed, H, frames):
    masks, off, K = FR.random_pack(seed, H, frames, K_choices=(1, 2, 3, 5, 64))
    want = FR.fuse_ref(masks.tolist(), off, K.tolist())
    tab = fu.FuseTables(K, off).to(engine)
    a = fu.download(fu.fuse_tables(engine, dev_masks(masks), tab))
    b = fu.download(fu.fuse_tables(engine, dev_masks(masks), tab))
    assert FR.same(a, want) is None, FR.same(a, want)
    assert all(a[k].tobytes() == b[k].tobytes() and a[k].dtype == b[k].dtype for k in a)
    host_tables = fu.fuse_host(masks, off, K)
    assert FR.same(a, host_tables) is None and all(a[k].dtype == host_tables[k].dtype for k in FR.EXACT)


# ------------------------------------------------------------------------------------------------ end to end
def frames_to_turns(sp, K, names):
    out = TC.truth_turns(sp, K)
    return [(a, b, names[int(n[1:])]) for a, b, n in out]


@functools.lru_cache(maxsize=None)
def public_case():
    """hypotheses[r] = (a result, a turn list, a result) over the edge frame counts; the turn list is a noisy copy under other names."""
    rng = np.random.default_rng(77)
    hyps, n_samples = [], []
    for r, G in enumerate(FR.EDGE_FRAMES):
        base = TC.runs_table(rng, G, 3) if G else np.zeros((0, 2), np.int32)
        noisy = []
        for c in range(2):
            sp = base.copy()
            for g in rng.choice(G, size=G // 8, replace=False) if G else []:
                sp[g, 0] = int(rng.integers(-1, 3))
            perm = rng.permutation(3)
            noisy.append(np.where(sp >= 0, perm[np.maximum(sp, 0)], -1).astype(np.int32))
        hyps.append([TC.result(base, 3), frames_to_turns(noisy[0], 3, ["zoe", "al", "kim"]), TC.result(noisy[1], 4)])
        n_samples.append(270 * G + 226 if G else 0)
    return hyps, n_samples


def fields(res):
    f = res.fusion
    return (res.speakers.tobytes(), res.turns, res.n_speakers, f["order"], f["weights"], f["dis"].tolist(), f["label_of"], f["speech"], f["overlap"],
            f["unanimous"], f["overflow"])


def test_public_calls_end_to_end(engine, monkeypatch):
    hyps, n_samples = public_case()
    before = [h[0].speakers.copy() for h in hyps]
    bk = sub("backend")
    be = bk.Backend()
    monkeypatch.setattr(be, "engine", lambda: engine)
    for kw in ({}, {"weights": [3, 1, 2], "max_speakers": 1}):
        want = TC.host_fuse(hyps, n_samples, **kw)
        got = fu.fuse_results(engine, hyps, n_samples, **kw)
        again = bk.fuse_diarizations(be, hyps, n_samples, **kw)
        assert len(got) == len(hyps) == 6
        for r, (g, w, a) in enumerate(zip(got, want, again)):
            assert fields(g) == fields(w) == fields(a), (r, kw)
            assert g.speakers.dtype == np.int32 and type(g) is type(w) and g is not hyps[r][g.fusion["order"][0]]
    assert got[0].turns == [] and any(x.fusion["unanimous"] < len(x.speakers) for x in got)
    assert all(np.array_equal(h[0].speakers, b) for h, b in zip(hyps, before))      # the inputs are left as they were
    # a recording without a result takes its grid from n_samples
    turns_only = [[h[1], h[1]] for h in hyps]
    for g, w in zip(fu.fuse_results(engine, turns_only, n_samples), TC.host_fuse(turns_only, n_samples)):
        assert fields(g) == fields(w) and isinstance(g, fu.FusedDiarization)
    # the pairwise part alone
    a, b = [h[2] for h in hyps], [h[1] for h in hyps]
    cmp1 = fu.compare(engine, a, b, n_samples)
    cmp2 = bk.compare_diarizations(be, a, b, n_samples)
    for r, (x, y) in enumerate(zip(cmp1, cmp2)):
        assert sorted(x) == sorted(y) == sorted(["co", "mapping", "names_a", "names_b", "sum_max", "sum_min", "correct", "disagreement", "unanimous"])
        assert all(np.array_equal(x[k], y[k]) for k in x), r
        der = sc.score_host(a[r].speakers, n_samples[r], b[r])
        kd = der.co.shape[1]                                                     # score_host counts a's speakers up to the largest one named
        assert x["correct"] == der.correct and np.array_equal(x["co"][:kd].T, der.co) and not x["co"][kd:].any(), r
        assert x["disagreement"] == ((x["sum_max"] - x["correct"]) / x["sum_max"] if x["sum_max"] else 0.0)
        assert int(x["co"][np.arange(4)[x["mapping"] >= 0], x["mapping"][x["mapping"] >= 0]].sum()) == x["correct"]
        assert x["names_a"] is None and x["names_b"] == sc.prepare_reference(b[r])[1]
    single = bk.compare_diarizations(be, a[5], b[5], n_samples[5])
    assert single["correct"] == cmp1[5]["correct"] and np.array_equal(single["co"], cmp1[5]["co"])


# ------------------------------------------------------------------------------------------------ refusals
def with_tables(tab, **tensors):
    t = copy.copy(tab)
    for name, v in tensors.items():
        setattr(t, name + "_d", v)
    return t


def test_argument_faults_of_every_wrapper(engine, monkeypatch):
    masks, off, K, _ = edge_pack(3)
    tab = fu.FuseTables(K, off).to(engine)
    m_d = dev_masks(masks)
    sp = dev(np.random.default_rng(1).integers(-1, 6, (tab.G, 2)).astype(np.int32))
    offs = dict(frame_off=tab.frame_off_d, spk_off=tab.spk_off_d, co_off=tab.co_off_d)
    split = lambda a: ({k: v for k, v in a.items() if k not in offs}, with_tables(tab, **{k: v for k, v in a.items() if k in offs}))  # noqa: E731

    def masks_call(_, **a):
        rest, t = split(a)
        return fu.fuse_masks(engine, rest["speakers"], t, 1, out=rest["out"].clone() if rest["out"].is_cuda and rest["out"].is_contiguous() else rest["out"])
    OA.exercise(engine, monkeypatch, masks_call, dict(speakers=sp, out=torch.zeros(tab.G, dtype=torch.int64, device="cuda"), **offs),
                {"speakers": lambda t: t[:-1]})

    def cooccur_call(_, **a):
        rest, t = split(a)
        return fu.fuse_cooccur(engine, rest["mask"], t)
    OA.exercise(engine, monkeypatch, cooccur_call, dict(mask=m_d, **offs))
    co, tally = fu.fuse_cooccur(engine, m_d, tab)

    def map_call(_, co, row_off, col_off):
        return fu.pair_map(engine, co, with_tables(tab, row_off=row_off, col_off=col_off))[1]      # the map itself is any optimal one, and unique here too
    OA.exercise(engine, monkeypatch, map_call, dict(co=co, row_off=tab.row_off_d, col_off=tab.col_off_d))
    _, correct = fu.pair_map(engine, co, tab)

    def labels_call(_, co, tally, correct, weights, rank_weight, **a):
        return fu.fuse_labels(engine, co, tally, correct, with_tables(tab, rank_weight=rank_weight, **a), weights)
    OA.exercise(engine, monkeypatch, labels_call, dict(co=co, tally=tally, correct=correct, weights=dev(np.asarray([4, 5, 6], np.int32)),
                                                       rank_weight=tab.rank_weight_d, **offs))
    _, _, weight, label_of, _, overflow = fu.fuse_labels(engine, co, tally, correct, tab)

    def vote_call(_, mask, label_of, weight, overflow, **a):
        return fu.fuse_vote(engine, mask, label_of, weight, overflow, with_tables(tab, **a), 2)
    OA.exercise(engine, monkeypatch, vote_call, dict(mask=m_d, label_of=label_of, weight=weight, overflow=overflow, **offs))


def test_the_library_refuses_on_its_own(engine):
    lib, ctx = engine.lib, engine.ctx
    masks, off, K = FR.case_greedy_tie()
    tab = fu.FuseTables(K, off).to(engine)
    m_d = dev_masks(masks)
    co = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    tally = torch.full((1, 2), -7, dtype=torch.int64, device="cuda")
    cooccur = lambda H, G, mx: lib.sdk_fuse_cooccur(ctx, m_d.data_ptr(), tab.frame_off_d.data_ptr(), tab.spk_off_d.data_ptr(), tab.co_off_d.data_ptr(),  # noqa: E731
                                                    H, 1, G, mx, 4, co.data_ptr(), tally.data_ptr(), None)
    assert cooccur(1, 6, 2) != 0 and b"H=1" in lib.sdk_last_error()
    assert cooccur(9, 6, 2) != 0 and b"H=9" in lib.sdk_last_error()
    assert cooccur(2, 1 << 30, 2) != 0 and b"fewer than 2^30" in lib.sdk_last_error()
    assert cooccur(2, -1, 2) != 0 and b"fewer than 2^30" in lib.sdk_last_error()
    assert cooccur(2, 6, 65) != 0 and b"65 speakers" in lib.sdk_last_error()
    sp = torch.full((6, 2), -7, dtype=torch.int32, device="cuda")
    tallies = torch.full((1, 4), -7, dtype=torch.int64, device="cuda")
    lab, w, ov = (torch.zeros(4, dtype=torch.int32, device="cuda") for _ in range(3))
    vote = lambda cap: lib.sdk_fuse_vote(ctx, m_d.data_ptr(), tab.frame_off_d.data_ptr(), tab.spk_off_d.data_ptr(), lab.data_ptr(), w.data_ptr(), ov.data_ptr(),  # noqa: E731
                                         2, 1, 6, 2, cap, sp.data_ptr(), tallies.data_ptr(), None)
    assert vote(0) != 0 and b"cap=0" in lib.sdk_last_error() and vote(3) != 0 and b"cap=3" in lib.sdk_last_error()
    assert lib.sdk_fuse_masks(ctx, sp.data_ptr(), tab.frame_off_d.data_ptr(), tab.spk_off_d.data_ptr(), 1, 6, 65, m_d.data_ptr(), None) != 0
    assert b"65 speakers" in lib.sdk_last_error()
    rc = lib.sdk_fuse_labels(ctx, co.data_ptr(), tally.data_ptr(), tally.data_ptr(), tab.spk_off_d.data_ptr(), tab.co_off_d.data_ptr(), tab.rank_weight_d.data_ptr(),
                             None, 9, 1, 2, tallies.data_ptr(), lab.data_ptr(), lab.data_ptr(), lab.data_ptr(), lab.data_ptr(), lab.data_ptr(), None)
    assert rc != 0 and b"H=9" in lib.sdk_last_error()
    with pytest.raises(LIB.SdkError, match="H=9"):
        LIB.check(rc, "sdk_fuse_labels")
    torch.cuda.synchronize()                                                     # every refusal came before the first write
    assert (host(co) == -7).all() and (host(tally) == -7).all() and (host(sp) == -7).all() and (host(tallies) == -7).all()
    assert np.array_equal(host(m_d).view(np.uint64), masks)
    # no frames at all: the accumulators are cleared, the labels are made, and nothing else is read
    empty = fu.FuseTables([[2, 0], [1, 3]], [0, 0, 0]).to(engine)
    out = fu.download(fu.fuse_tables(engine, torch.zeros((2, 0), dtype=torch.int64, device="cuda"), empty))
    want = FR.fuse_ref([[], []], [0, 0, 0], [[2, 0], [1, 3]])
    assert FR.same(out, want) is None and out["n_labels"].tolist() == [3, 3] and out["speakers"].shape == (0, 2)
