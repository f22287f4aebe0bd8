"""CPU twin of test_diarize_grouped_edges_gpu.py: every case builder of tests/grouped_ref.py against the package's host restatements AND the
per-recording references, and every fixture condition (bit-equal tie cosines, margins, shares kept, the presence of every constructed
class) on the references alone."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grouped_ref as GR  # noqa: E402
import test_diarize_many_cpu as MC  # noqa: E402

dz = GR.dz
TABLES = GR.group_tables()
STEPS, MAXSP = [0.5, 1.0, 2.5], [None, 0, 1, 2, 5]


def test_group_tables_enter_every_class():
    cls = {name: GR.table_classes(c) for name, c in TABLES.items()}
    assert {c["R"] for c in cls.values()} >= {1, 7, 300}
    for key in ("empty_first", "empty_last", "two_empty", "at_64", "at_256", "at_255", "at_257", "second_block"):
        assert any(c[key] for c in cls.values()), key
    assert set(np.unique(TABLES["R300"])) == {1, 2, 3}


# ------------------------------------------------------------------------------------------------ reconstruct
def reconstruct_host_equals_reference(pack, maxsp):
    ref = GR.reconstruct_reference(pack, maxsp)
    count, speakers, acts = dz.reconstruct_grouped_host(pack["cls"], np.concatenate(pack["starts"]), pack["labels"], pack["chunk_off"],
                                                        pack["frame_off"], pack["n"], pack["cent_off"], maxsp)
    assert np.array_equal(count, ref[0]) and np.array_equal(speakers, ref[1])
    assert all(np.array_equal(a, b) for a, b in zip(acts, ref[2])) and len(acts) == len(ref[2])
    for r, n in enumerate(pack["n"]):                                     # the single-recording restatement too
        a, b, g0, g1 = int(pack["chunk_off"][r]), int(pack["chunk_off"][r + 1]), int(pack["frame_off"][r]), int(pack["frame_off"][r + 1])
        c1, s1, a1, _ = dz.reconstruct_host(pack["cls"][a:b], pack["starts"][r], pack["labels"][a:b], max(pack["K_list"][r], 1), int(n), maxsp)
        assert np.array_equal(c1, ref[0][g0:g1]) and np.array_equal(s1, ref[1][g0:g1]) and np.array_equal(a1, ref[2][r])
    return ref


@pytest.mark.parametrize("step_s", STEPS)
@pytest.mark.parametrize("maxsp", MAXSP)
def test_reconstruct_edges_host_equals_the_reference(step_s, maxsp):
    pack = GR.reconstruct_edges(step_s)
    assert np.diff(pack["frame_off"]).tolist()[:6] == [257, 1, 255, 256, 0, 40] and pack["K_list"][:6] == [0, 1, 64, 65, 3, 200]
    count, _, _ = reconstruct_host_equals_reference(pack, maxsp)
    _, nc = GR.mean_counts(pack["cls"][int(pack["chunk_off"][6]):], pack["starts"][6], int(np.diff(pack["frame_off"])[6]))
    assert 10 / step_s <= nc.max() <= 10 / step_s + 1 and nc.min() == 0   # a frame is seen by up to 20, 10 or 4 chunks (and the one that ends the recording), the last by none
    assert int(count.max()) == (2 if maxsp is None else min(2, maxsp))


@pytest.mark.parametrize("step_s", STEPS)
@pytest.mark.parametrize("maxsp", MAXSP)
def test_reconstruct_constructed_host_equals_the_reference(step_s, maxsp):
    pack = GR.reconstruct_constructed(step_s)
    count, speakers, acts = reconstruct_host_equals_reference(pack, maxsp)
    lab0 = pack["labels"][:int(pack["chunk_off"][1])]
    assert (lab0 == 3).any() and (lab0 == 8).any() and any(len(set(row)) < 3 for row in lab0.tolist())      # K_r, K_r + 5, a repeated label
    a, b = int(pack["chunk_off"][1]), int(pack["chunk_off"][2])
    assert (pack["labels"][a:b] == -1).all() and (acts[1] == 0).all() and (speakers[int(pack["frame_off"][1]):int(pack["frame_off"][2])] == -1).all()
    assert pack["frame_off"][3] == pack["frame_off"][2] and (pack["labels"][int(pack["chunk_off"][3]):] >= 4).any()
    G0 = int(pack["frame_off"][1])
    cnt, nc = GR.mean_counts(pack["cls"][:int(pack["chunk_off"][1])], pack["starts"][0], G0)
    p, act = pack["planted"][0], acts[0]
    assert all(len(p[k]) >= 1 for k in ("half", "one_and_half", "tie2", "tie3")), {k: len(v) for k, v in p.items()}
    cap = 2 if maxsp is None else min(2, maxsp)
    for g in p["half"]:
        assert nc[g] % 2 == 0 and 2 * cnt[g] == nc[g] and count[g] == min(1, cap)                     # exactly 0.5 rounds up
    for g in p["one_and_half"]:
        assert 2 * cnt[g] == 3 * nc[g] and count[g] == min(2, cap)                                    # exactly 1.5 rounds up
    for g in p["tie2"]:
        assert act[g, 0] == act[g, 1] == nc[g] > act[g, 2] and speakers[g].tolist() == [0, 1][:cap] + [-1] * (2 - cap)
    for g in p["tie3"]:
        assert act[g, 0] == act[g, 1] == act[g, 2] > 0 and count[g] == min(2, cap) and speakers[g].tolist() == [0, 1][:cap] + [-1] * (2 - cap)


@pytest.mark.parametrize("name", list(TABLES))
def test_reconstruct_group_tables_host_equals_the_reference(name):
    pack = GR.reconstruct_tables(TABLES[name])
    assert np.array_equal(pack["frame_off"], GR.offsets(TABLES[name]))
    reconstruct_host_equals_reference(pack, None)


def test_reconstruct_host_on_a_frame_table_longer_than_the_recording():
    pack = GR.reconstruct_tables([30, 5, 12])
    ref = GR.reconstruct_reference(pack, None)
    long_off = GR.offsets([30 + 9, 5, 12 + 300])
    count, speakers, _ = dz.reconstruct_grouped_host(pack["cls"], np.concatenate(pack["starts"]), pack["labels"], pack["chunk_off"], long_off,
                                                     pack["n"], pack["cent_off"], None)
    for r, extra in enumerate((9, 0, 300)):
        g0, g1, G = int(long_off[r]), int(long_off[r + 1]), int(np.diff(pack["frame_off"])[r])
        assert np.array_equal(count[g0:g0 + G], ref[0][int(pack["frame_off"][r]):int(pack["frame_off"][r + 1])])
        assert (count[g0 + G:g1] == 0).all() and (speakers[g0 + G:g1] == -1).all() and g1 - g0 - G == extra


# ------------------------------------------------------------------------------------------------ assign
@pytest.mark.parametrize("d", [64, 512])
@pytest.mark.parametrize("constrained", [0, 1])
def test_assign_edges_host_equals_the_reference(d, constrained):
    (E, info, cent, chunk_off, cent_off, _), refs = GR.assign_reference(d, constrained)
    assert np.diff(cent_off).tolist() == [0, 64, 65, 300, 2] and np.diff(chunk_off)[[0, 4]].tolist() == [0, 0] and np.isnan(E).any()
    labels, score = dz.assign_grouped_host(E, info, cent, chunk_off, cent_off, bool(constrained))
    total, kept, err = GR.check_assign(d, refs, chunk_off, labels, score, 1e-12)
    print(f"assign edges d={d} constrained={constrained}: {total} chunks with candidates, {total - kept} left out, host score error {err:.3e}")
    assert max(int(r["labels"].max(initial=-1)) for r in refs) >= 256    # a label past the first 256 clusters is in use


# ------------------------------------------------------------------------------------------------ fold
@pytest.mark.parametrize("d", [64, 512])
def test_fold_edges_host_equals_fold_small_clusters(d):
    cases = GR.fold_edges(d)
    cent, sizes, cl_off, eff, cent_off, ref, margins = MC.fold_tables(cases)
    print(f"fold edges d={d}: least best-minus-second cosine {min(margins):.3e}")
    assert min(margins) > 1e-9
    assert np.diff(cent_off).tolist() == [3, 130, 1, 1] and eff.tolist() == [2, 3, 3, 1]
    b = int(cl_off[1])
    small = np.flatnonzero(sizes[b:b + 136] < 3)
    assert small.tolist() == sorted(GR.PLANT) and set(sizes[b:b + 136].tolist()) == {2, 3}     # sizes exactly eff - 1 (folds) and eff (stays)
    lab = cases[1][1]
    for s, t in GR.PLANT.items():                                        # the reference sends every small cluster where it was planted
        assert set(ref[1][lab == s]) == set(ref[1][lab == t])
    assert {t // 64 for t in GR.PLANT.values()} == {0, 1, 2}
    remap = dz.fold_grouped_host(cent, sizes, cl_off, eff, cent_off)
    for r, (_, lab, _) in enumerate(cases):
        assert np.array_equal(remap[int(cl_off[r]) + lab] - cent_off[r], ref[r])


def test_fold_many_host_equals_fold_small_clusters():
    cases = GR.fold_many(64)
    cent, sizes, cl_off, eff, cent_off, ref, margins = MC.fold_tables(cases)
    assert len(cases) == 300 and set(np.diff(cl_off)) == {1, 2, 3} and min(margins) > 1e-9 and (eff == 2).all()
    assert (np.diff(cent_off) < np.diff(cl_off)).sum() >= 100              # recordings in which a cluster folds
    remap = dz.fold_grouped_host(cent, sizes, cl_off, eff, cent_off)
    for r, (_, lab, _) in enumerate(cases):
        assert np.array_equal(remap[int(cl_off[r]) + lab] - cent_off[r], ref[r])


@pytest.mark.parametrize("name", list(TABLES))
def test_fold_group_tables_host_equals_fold_small_clusters(name):
    cases = GR.fold_tables_case(TABLES[name])
    cent, sizes, cl_off, eff, cent_off, ref, margins = GR.fold_pack(cases, MC.fold_tables)
    assert np.array_equal(cl_off, GR.offsets(TABLES[name])) and (not margins or min(margins) > 1e-9)
    folds = int((sizes < np.repeat(eff, np.diff(cl_off))).sum())
    assert folds >= 1 or name in ("R300",), name                          # 1 - 3 clusters: the effective minimum stays 1 unless a large cluster is there
    remap = dz.fold_grouped_host(cent, sizes, cl_off, eff, cent_off)
    for r, case in enumerate(cases):
        if case is not None:
            assert np.array_equal(remap[int(cl_off[r]) + case[1]] - cent_off[r], ref[r])


@pytest.mark.parametrize("d", [64, 512])
def test_fold_exact_ties_and_nan_on_the_host(d):
    cent, sizes, cl_off, eff, cent_off, target, names = GR.fold_exact(d)
    assert names == ["lanes_uv", "lanes_vu", "same_lane_uv", "same_lane_vu", "one_nan", "all_nan"]
    norms = np.array([GR.chain(c, c) for c in cent[~np.isnan(cent).any(1)]])
    assert (norms == 1.0).all()                                          # unit length, exactly
    for r, (name, gap) in enumerate(zip(names[:4], (1, 1, 64, 64))):
        b = int(cl_off[r])
        cos = np.array([GR.chain(cent[b], cent[j]) for j in range(b + 2, int(cl_off[r + 1]))])
        j = int(target[b]) - b - 2
        assert cos[j] == cos[j + gap] == 0.5 and cos[j].tobytes() == cos[j + gap].tobytes(), name      # bit-equal
        assert not np.array_equal(cent[b + 2 + j], cent[b + 2 + j + gap]) and (np.delete(cos, [j, j + gap]) < 0.5).all()
        assert (j % 64 == (j + gap) % 64) == (gap == 64)                 # the same lane, or two lanes
    b = int(cl_off[4])
    assert np.isnan(GR.chain(cent[b], cent[b + 2 + 5])) and np.isnan(cent[b:int(cl_off[5])]).sum() == 1
    b, e = int(cl_off[5]), int(cl_off[6])
    assert all(np.isnan(GR.chain(cent[k], cent[j])) for k in (b, b + 1) for j in range(b + 2, e)) and target[b] == b + 2
    large = sizes >= np.repeat(eff, np.diff(cl_off))
    assert np.array_equal(target[large], np.flatnonzero(large))
    remap = dz.fold_grouped_host(cent, sizes, cl_off, eff, cent_off)
    assert np.array_equal(remap, GR.number_kept(target, cl_off, cent_off))


def test_cut_holds_entries_outside_the_clusters():
    for n in (0, 255, 256, 257):
        cut = GR.cut_for(100, n)
        assert len(cut) == n and (n == 0 or ((cut == -1).any() and (cut == 100).any() and (cut > 100).any()))


# ------------------------------------------------------------------------------------------------ first seen / renumber
def renumber_host_equals_reference(tabs, frame_off, cent_off, C):
    first = dz.first_seen_host(np.concatenate(tabs), frame_off, cent_off)
    chunk_off, labels = GR.labels_for(C, cent_off)
    c32, c64 = GR.odd_centroids(int(cent_off[-1]), 8)
    renum, lab2, src = GR.renumber_expected(tabs, cent_off, chunk_off, labels)
    h_renum, h_lab, h64 = dz.renumber_host(first, cent_off, chunk_off, labels, c64)
    assert np.array_equal(h_renum, renum) and np.array_equal(h_lab, lab2) and np.array_equal(h64.view(np.int64), c64[src].view(np.int64))
    return first, renum, labels, lab2


@pytest.mark.parametrize("C", [0, 85, 86])
def test_first_seen_and_renumber_edges_host_equal_order_by_appearance(C):
    tabs, frame_off, cent_off, names = GR.speakers_edges()
    first, renum, labels, lab2 = renumber_host_equals_reference(tabs, frame_off, cent_off, C)
    per = {n: (first[int(cent_off[r]):int(cent_off[r + 1])], renum[int(cent_off[r]):int(cent_off[r + 1])]) for r, n in enumerate(names)}
    assert per["both_slots_new"][0].tolist() == [15, 7, 6, GR.I32_MAX] and per["both_slots_new"][1].tolist() == [2, 1, 0, 3]
    assert (per["never_seen"][0] == GR.I32_MAX).all() and per["never_seen"][1].tolist() == [0, 1, 2, 3, 4]
    assert (per["no_frames"][0] == GR.I32_MAX).all() and per["no_frames"][1].tolist() == [0, 1, 2]
    assert per["contention"][0].tolist() == [2001, 0]
    for n, K in (("K257", 257), ("K300", 300)):
        never = int((per[n][0] == GR.I32_MAX).sum())
        assert len(per[n][0]) == K and 0.4 * K <= never <= 0.6 * K and sorted(per[n][1]) == list(range(K))
    if C:
        K_of = np.repeat(np.diff(cent_off), np.diff(GR.labels_for(C, cent_off)[0]))[:, None]
        assert (labels >= K_of).any() and np.array_equal(lab2[labels >= K_of], labels[labels >= K_of]) and (lab2 != labels).any()
    assert 3 * 85 < 256 < 3 * 86


@pytest.mark.parametrize("name", list(TABLES))
def test_first_seen_and_renumber_group_tables_on_the_host(name):
    counts = TABLES[name]
    rng = np.random.default_rng(7)
    tabs, frame_off, cent_off = GR.speakers_tables(counts, rng.integers(0, 5, len(counts)))        # the table counts the frames
    renumber_host_equals_reference(tabs, frame_off, cent_off, 40)
    tabs, frame_off, cent_off = GR.speakers_tables(rng.integers(0, 9, len(counts)), counts)        # the table counts the clusters
    renumber_host_equals_reference(tabs, frame_off, cent_off, 40)
