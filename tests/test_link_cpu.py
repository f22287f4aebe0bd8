"""CPU checks of the speaker linking across recordings: tests/link_ref.py (the float64 restatement of the linked centroid linkage, forbiddance by
member sets) against scipy, against the constraint and against the stop rule; the host rules of diarize.link_speakers and cluster.link_rows on
hand-made results with a provider built on that restatement; Backend.link_speakers' refusals."""
import numpy as np
import pytest
import torch
from scipy.cluster.hierarchy import linkage

import ahc_ref
import link_ref
from conftest import sub
from oracle.spectral import vmf_mixture

CL = sub("cluster")
DZ = sub("diarize")


def _same_linkage(Z, Zs):
    assert Z.shape == Zs.shape, (Z.shape, Zs.shape)
    assert np.array_equal(Z[:, [0, 1, 3]], Zs[:, [0, 1, 3]]), "ids / counts differ"
    np.testing.assert_allclose(Z[:, 2], Zs[:, 2], rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("N,k,noise", [(300, 6, 0.45), (150, 0, 0.0)])
def test_ref_without_groups_equals_scipy(N, k, noise):
    if k:
        X = vmf_mixture(N, 192, k, 11 + N, noise)[0]
    else:
        X = np.random.default_rng(5).standard_normal((N, 192))
        X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    Z, m, gaps = link_ref.linked_linkage(X, np.full(N, -1))
    assert m == N - 1 and gaps.min() > 1e4 * 1e-12
    _same_linkage(Z, linkage(X.astype(np.float64), "centroid"))
    Za, _ = ahc_ref.centroid_linkage(X)                # and the lazy restatement of the unconstrained kernel, bit for bit
    assert np.array_equal(Z, Za)


@pytest.mark.parametrize("N", [3, 17, 64, 65, 129])
def test_ref_with_groups_never_joins_a_group(N):
    X, group, _ = link_ref.planted(N, 32, N)
    Z, m, gaps = link_ref.linked_linkage(X, group)
    assert m < N - 1 or N <= 3 or len(np.unique(group)) == N, "the constraint must end the run early"
    assert np.all(Z[m:] == 0) and np.all(Z[:m, 3] >= 2)
    ahc_like = Z[:m]
    assert np.all(ahc_like[:, 0] < ahc_like[:, 1])
    for t in range(m + 1):                             # at EVERY step, not only at the end
        assert link_ref.no_group_twice(link_ref.labels_after(Z, N, t), group), t
    # the end is the constraint's: every pair of final clusters shares a group
    lab = link_ref.labels_after(Z, N, m)
    sets = [set(group[lab == c].tolist()) for c in range(lab.max() + 1)]
    assert all(sets[a] & sets[b] for a in range(len(sets)) for b in range(a + 1, len(sets)))
    # and it differs from the free linkage, which ends in one cluster
    assert m == N - len(sets)


def test_ref_stop_truncates_at_cut_level():
    X, group, _ = link_ref.planted(90, 32, 4)
    Zf, mf, _ = link_ref.linked_linkage(X, group)
    hs = np.sort(Zf[:mf, 2])
    for t in (0.0, float(hs[0]), float(hs[len(hs) // 3]) * (1 + 1e-9), 0.2, float(hs[-1]), 10.0, np.inf):
        Z, m, _ = link_ref.linked_linkage(X, group, t)
        assert m == CL.cut_level(Zf[:mf], t), t
        assert np.array_equal(Z[:m], Zf[:m]) and np.all(Z[m:] == 0)


# ------------------------------------------------------------------------------------------------ cluster.link_rows
def test_link_rows_small_and_labels():
    P = link_ref.RefProvider()
    r0 = CL.link_rows(P, torch.zeros((0, 8)), np.zeros(0, np.int32), 0.5)
    assert r0.labels.shape == (0,) and r0.linkage.shape == (0, 4) and r0.n_merges == 0
    r1 = CL.link_rows(P, torch.ones((1, 8)), np.zeros(1, np.int32), 0.5)
    assert np.array_equal(r1.labels, [0]) and r1.n_merges == 0
    X, group, _ = link_ref.planted(40, 32, 9)
    Z, m, _ = link_ref.linked_linkage(X, group, 0.3)
    res = CL.link_rows(P, torch.from_numpy(X), group, 0.3)
    assert res.n_merges == m and np.array_equal(res.linkage, Z)
    assert np.array_equal(res.labels, link_ref.labels_after(Z, 40, m)) and res.labels.dtype == np.int32
    with pytest.raises(ValueError, match="group must be"):
        CL.link_rows(P, torch.from_numpy(X), group[:-1], 0.3)
    with pytest.raises(ValueError, match="threshold=-1"):
        CL.link_rows(P, torch.from_numpy(X), group, -1.0)


# ------------------------------------------------------------------------------------------------ diarize.link_speakers, host rules
def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return (v / np.linalg.norm(v)).astype(np.float32)


def _result(cents, turns):
    cents = np.asarray(cents, dtype=np.float32).reshape(len(cents), 4)
    return DZ.DiarizationResult(turns=turns, n_speakers=len(cents), centroids=cents, labels=np.zeros((0, 3), np.int32), count=np.zeros(0, np.uint8),
                                speakers=np.zeros((0, 2), np.int32), starts=np.zeros(0, np.int64), info=np.zeros((0, 3, 4), np.int32))


E0, E1, E2, E3 = np.eye(4)
A = lambda e: _unit(E0 + e * E3)      # noqa: E731  person A seen with a small offset
B = lambda e: _unit(E1 + e * E3)      # noqa: E731
Cc = lambda e: _unit(E2 + e * E3)     # noqa: E731


def _scene():
    """rec 0: B, A; rec 1: empty; rec 2: A, C, B(short); rec 3: C."""
    r0 = _result([B(0.00), A(0.02)], [(0.0, 5.0, 0), (5.0, 9.0, 1)])
    r1 = _result(np.zeros((0, 4)), [])
    r2 = _result([A(0.05), Cc(0.01), B(0.08)], [(0.0, 4.0, 0), (4.0, 8.0, 1), (8.0, 8.5, 2), (9.0, 9.25, 2)])
    r3 = _result([Cc(0.06)], [(1.0, 3.0, 0)])
    return [r0, r1, r2, r3]


def test_link_speakers_numbering_by_first_appearance_and_empty_recordings():
    res = _scene()
    links = DZ.link_speakers(link_ref.RefProvider(), res, threshold=0.3)
    assert [a.tolist() for a in links.ids] == [[0, 1], [], [1, 2, 0], [2]]
    assert all(a.dtype == np.int32 for a in links.ids) and links.n_global == 3 and links.n_merges == 3
    assert links.profile.tolist() == [-1, -1, -1] and links.names is None
    want = np.stack([_unit(B(0.0).astype(np.float64) + B(0.08)), _unit(A(0.02).astype(np.float64) + A(0.05)), _unit(Cc(0.01).astype(np.float64) + Cc(0.06))])
    assert links.centroids.dtype == np.float32 and np.abs(links.centroids - want).max() < 1e-6
    assert links.linkage.shape == (5, 4) and np.all(links.linkage[3:] == 0)
    # the rows offered are the results' centroids in order: equal to the restatement on them
    X = np.concatenate([r.centroids for r in res])
    Z, m, _ = link_ref.linked_linkage(X, [0, 0, 2, 2, 2, 3], 0.3)
    assert np.array_equal(links.linkage, Z) and m == 3
    # nothing to link
    none = DZ.link_speakers(link_ref.RefProvider(), [], threshold=0.3)
    assert none.ids == [] and none.n_global == 0 and none.centroids.shape == (0, 0) and none.linkage.shape == (0, 4)
    only_empty = DZ.link_speakers(link_ref.RefProvider(), [res[1], res[1]], threshold=0.3)
    assert [a.tolist() for a in only_empty.ids] == [[], []] and only_empty.n_global == 0


def test_link_speakers_same_recording_never_joins():
    r0 = _result([A(0.0), A(0.01)], [(0.0, 5.0, 0), (5.0, 9.0, 1)])       # two near-identical centroids in ONE recording
    r1 = _result([A(0.02)], [(0.0, 5.0, 0)])
    links = DZ.link_speakers(link_ref.RefProvider(), [r0, r1], threshold=0.5)
    assert [a.tolist() for a in links.ids] == [[0, 1], [1]] and links.n_global == 2      # a1-b joins first (0.01 < 0.02); then a0 is barred


def test_link_speakers_min_speech_singletons():
    res = _scene()
    links = DZ.link_speakers(link_ref.RefProvider(), res, threshold=0.3, min_speech_s=1.0)     # rec 2's speaker 2 has 0.75 s
    assert [a.tolist() for a in links.ids] == [[0, 1], [], [1, 2, 3], [2]] and links.n_global == 4
    assert links.linkage.shape == (4, 4) and links.n_merges == 2                                  # five rows were offered
    assert np.abs(links.centroids[3] - B(0.08)).max() < 1e-7 and np.abs(links.centroids[0] - B(0.0)).max() < 1e-7
    exact = DZ.link_speakers(link_ref.RefProvider(), res, threshold=0.3, min_speech_s=0.75)     # "less than": 0.75 s is enough
    assert [a.tolist() for a in exact.ids] == [[0, 1], [], [1, 2, 0], [2]]
    with pytest.raises(ValueError, match="min_speech_s=-1"):
        DZ.link_speakers(link_ref.RefProvider(), res, min_speech_s=-1.0)


def test_link_speakers_profiles():
    res = _scene()
    # profile 0 = C, profile 1 = nobody heard (E3), profile 2 = A, profile 3 = a voice 0.16 from A's cluster: under the threshold, but A's cluster
    # holds profile 2 by then
    prof = np.stack([Cc(0.0), _unit(E3), A(0.03), A(0.2)])
    links = DZ.link_speakers(link_ref.RefProvider(), res, threshold=0.3, profiles=prof)
    assert [a.tolist() for a in links.ids] == [[0, 1], [], [1, 2, 0], [2]] and links.n_global == 3      # the profile-only clusters get no id
    assert links.profile.dtype == np.int32 and links.profile[0] == -1 and links.profile[2] == 0
    assert links.profile[1] == 2                                                                         # two profiles never share a cluster
    lab = link_ref.labels_after(links.linkage, 10, links.n_merges)
    assert len({int(l) for l in lab[6:]}) == 4, "every profile row sits in a cluster of its own"
    # the centroid mean leaves the profile rows out
    want = _unit(A(0.02).astype(np.float64) + A(0.05))
    assert np.abs(links.centroids[1] - want).max() < 1e-6
    with pytest.raises(ValueError, match="different widths"):
        DZ.link_speakers(link_ref.RefProvider(), res, profiles=np.zeros((2, 5), np.float32))
    # one voice enrolled twice: each enrolment takes the nearer recording, and the two clusters can then never meet
    twice = DZ.link_speakers(link_ref.RefProvider(), res, threshold=0.3, profiles=np.stack([A(0.03), A(0.04)]))
    assert [a.tolist() for a in twice.ids] == [[0, 1], [], [2, 3, 0], [3]] and twice.profile.tolist() == [-1, 0, 1, -1]
    # profiles alone
    alone = DZ.link_speakers(link_ref.RefProvider(), [], threshold=0.3, profiles=prof)
    assert alone.n_global == 0 and alone.ids == [] and alone.n_merges == 0


def test_relabel_turns():
    res = _scene()
    links = DZ.link_speakers(link_ref.RefProvider(), res, threshold=0.3)
    assert DZ.relabel_turns(res[2], links.ids[2]) == [(0.0, 4.0, 1), (4.0, 8.0, 2), (8.0, 8.5, 0), (9.0, 9.25, 0)]
    assert DZ.relabel_turns(res[1], links.ids[1]) == []
    two = _result([A(0.0), B(0.0)], [(0.0, 2.0, 0), (0.0, 2.0, 1)])
    assert DZ.relabel_turns(two, np.array([5, 3])) == [(0.0, 2.0, 3), (0.0, 2.0, 5)]                     # by start, then global speaker


# ------------------------------------------------------------------------------------------------ Backend.link_speakers
def test_backend_link_speakers_names_from_candidates(monkeypatch):
    """candidates -> one row per enrolled speaker (the float64 mean of their unit embeddings, re-normalised), names on the result.  The store
    and the engine are stood in for: the batch is hand-made and the provider is the restatement."""
    for k in ("SDK_NO_TORCH", "SDK_COHORT", "SDK_COHORT_THRESHOLD"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SDK_MODEL", "resnet34")
    be = sub("backend").Backend()

    class Batch:
        speaker_ids = ["carol", "alice", "carol"]
        matrix = np.stack([2.0 * Cc(0.0), A(0.03), 3.0 * Cc(0.04)]).astype(np.float32)     # not unit: the rows are normalised before the mean

        def __len__(self):
            return 3
    monkeypatch.setattr(be, "_load_candidates", lambda c: Batch())
    monkeypatch.setattr(be, "engine", lambda: link_ref.RefProvider())
    links = be.link_speakers(_scene(), threshold=0.3, candidates=[{"id": "carol"}, {"id": "alice"}])
    assert [a.tolist() for a in links.ids] == [[0, 1], [], [1, 2, 0], [2]]
    assert links.names == [None, "alice", "carol"] and links.profile.tolist() == [-1, 1, 0]
    carol = _unit(Cc(0.0).astype(np.float64) + Cc(0.04))
    lab = link_ref.labels_after(links.linkage, 8, links.n_merges)
    assert lab[6] == lab[3] and lab[7] == lab[1]                     # rows 6, 7 are the profiles carol, alice
    Z, m, _ = link_ref.linked_linkage(np.concatenate([np.concatenate([r.centroids for r in _scene()]), np.stack([carol, A(0.03)])]),
                                      [0, 0, 2, 2, 2, 3, 4, 4], 0.3)
    # carol's row here is made from fp32 unit rows, the backend's from the scaled fp32 rows normalised in float64: they differ by fp32
    # rounding (2^-24 per coordinate, d = 4), so heights agree to 1e-6 and everything integral exactly
    assert m == links.n_merges and np.array_equal(Z[:, [0, 1, 3]], links.linkage[:, [0, 1, 3]]) and np.abs(Z[:, 2] - links.linkage[:, 2]).max() < 1e-6
    assert be.link_speakers(_scene(), threshold=0.3).names is None


# ------------------------------------------------------------------------------------------------ Backend.link_speakers' refusals
def test_backend_link_speakers_refusals(monkeypatch):
    for k in ("SDK_MODEL", "SDK_NO_TORCH", "SDK_COHORT", "SDK_COHORT_THRESHOLD"):
        monkeypatch.delenv(k, raising=False)
    be = sub("backend").Backend()                                     # ecapa
    with pytest.raises(ValueError, match="link_speakers: candidates.*'ecapa'.*SDK_MODEL=resnet34"):
        be.link_speakers(_scene(), candidates=[])
    monkeypatch.setenv("SDK_MODEL", "xvector")
    with pytest.raises(ValueError, match="'xvector'"):
        sub("backend").Backend().link_speakers([], candidates=[{"id": "x", "embeddings": []}])
    monkeypatch.setenv("SDK_MODEL", "ecapa")
    monkeypatch.setenv("SDK_NO_TORCH", "1")
    with pytest.raises(ValueError, match="link_speakers needs the torch engine: not available with SDK_NO_TORCH=1"):
        sub("backend").Backend().link_speakers(_scene())
