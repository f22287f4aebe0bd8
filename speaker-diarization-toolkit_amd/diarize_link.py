"""Speakers across recordings ("linking" in diarize.py's module docstring): one inventory for the results of many diarizations.  It reads
nothing of the pipeline but DiarizationResult.centroids and .turns; the linkage is cluster.link_rows.  diarize.py re-exports every name."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from .cluster import PYANNOTE_THRESHOLD, link_rows


@dataclass
class SpeakerLinks:
    ids: List[np.ndarray]                     # per recording, int32 [K_r]: the global speaker of every local speaker
    n_global: int
    centroids: np.ndarray                     # [n_global, d] unit fp32: float64 mean of the member unit centroids, re-normalised (profiles excluded)
    profile: np.ndarray                       # [n_global] int32: the row of `profiles` in the speaker's cluster, else -1
    linkage: np.ndarray                       # the merges made over the offered rows (cluster.LinkResult.linkage)
    n_merges: int
    names: Optional[list] = None              # Backend.link_speakers with candidates: [n_global] speaker_id or None


def link_speakers(eng, results, threshold: float = PYANNOTE_THRESHOLD, min_speech_s: float = 0.0, profiles=None) -> SpeakerLinks:
    """One speaker inventory for a list of DiarizationResult (Diarizer.run_many's, in order): which local speakers of different recordings are
    the same person.  Parity with any outside tool is unpinned; the tests pin this rule.

      rows       the `centroids` of every result, in recording order then local speaker order; the group of a row is its recording's index, so
                 two speakers of one recording - two different people, say the segmentation and the clustering - never share a global speaker
      min_speech_s  a local speaker whose turns total less than this many seconds is not offered to the linkage: it stays a speaker of its own
      profiles   [P, d] unit fp32, one row per enrolled speaker, appended after all recording rows with the one group R (the number of
                 recordings): no cluster ever holds two enrolled speakers
      linkage    cluster.link_rows (the linked centroid linkage on the device, csrc/ahc.hip) with stop = threshold
      numbering  global speakers are numbered by first appearance, in recording order then local speaker number; a cluster that holds only a
                 profile gets no id
      centroids  of a global speaker: the float64 mean of its members' unit centroids, re-normalised, stored fp32; a profile row is no member

    The default threshold is PyAnnote 3.1's WITHIN-recording value for single embeddings: it is untuned for centroids across recordings
    (averaged rows lie closer together than single ones do); pass a threshold chosen on your own data."""
    R = len(results)
    cents = [np.asarray(res.centroids, dtype=np.float32) for res in results]
    for r, c in enumerate(cents):
        if c.ndim != 2:
            raise ValueError(f"link_speakers: recording {r}: centroids must be [K, d], got {list(c.shape)}")
    prof = None if profiles is None else np.ascontiguousarray(profiles, dtype=np.float32)
    if prof is not None and prof.ndim != 2:
        raise ValueError(f"link_speakers: profiles must be [P, d], got {list(prof.shape)}")
    dims = {c.shape[1] for c in cents if c.shape[0]} | ({prof.shape[1]} if prof is not None and prof.shape[0] else set())
    if len(dims) > 1:
        raise ValueError(f"link_speakers: centroids and profiles of different widths {sorted(dims)}: one embedding space is needed")
    d = dims.pop() if dims else 0
    if not float(min_speech_s) >= 0.0:
        raise ValueError(f"link_speakers: min_speech_s={min_speech_s} (seconds, >= 0)")
    owner = [(r, k) for r in range(R) for k in range(cents[r].shape[0])]            # every local speaker, in numbering order
    offered = []
    for r, k in owner:
        total = sum(b - a for a, b, s in results[r].turns if s == k)
        offered.append(total >= float(min_speech_s))
    P = 0 if prof is None else int(prof.shape[0])
    rows = [cents[r][k] for (r, k), on in zip(owner, offered) if on] + [prof[p] for p in range(P)]
    group = [r for (r, _), on in zip(owner, offered) if on] + [R] * P
    n_rec = len(rows) - P
    if rows:
        E = torch.from_numpy(np.ascontiguousarray(np.stack(rows), dtype=np.float32))
        dev = getattr(eng, "device", None)
        link = link_rows(eng, E if dev is None else E.to(dev), np.asarray(group, np.int32), threshold)
    else:
        link = link_rows(eng, np.zeros((0, d), np.float32), np.zeros(0, np.int32), threshold)
    prof_of = {int(link.labels[n_rec + p]): p for p in range(P)}                    # cluster -> its profile row (at most one: they share a group)
    ids = [np.zeros(c.shape[0], np.int32) for c in cents]
    gid_of, members, profile = {}, [], []
    j = 0
    for (r, k), on in zip(owner, offered):
        c = None
        if on:
            c, j = int(link.labels[j]), j + 1
        if c is None or c not in gid_of:
            if c is not None:
                gid_of[c] = len(members)
            ids[r][k] = len(members)
            members.append([(r, k)])
            profile.append(prof_of.get(c, -1) if c is not None else -1)
        else:
            ids[r][k] = gid_of[c]
            members[gid_of[c]].append((r, k))
    out = np.zeros((len(members), d), np.float32)
    for gidx, m in enumerate(members):
        mean = np.stack([cents[r][k] for r, k in m]).astype(np.float64).mean(axis=0)
        out[gidx] = (mean / max(float(np.linalg.norm(mean)), 1e-12)).astype(np.float32)
    return SpeakerLinks(ids, len(members), out, np.asarray(profile, np.int32).reshape(-1), link.linkage, link.n_merges)


def relabel_turns(result, ids_r) -> List[Tuple[float, float, int]]:
    """A recording's turns with its local speakers replaced by their global ones (SpeakerLinks.ids[r]), by start then speaker."""
    ids_r = np.asarray(ids_r)
    return sorted(((a, b, int(ids_r[k])) for a, b, k in result.turns), key=lambda t: (t[0], t[2]))
