"""Multi-scale windows for the eigengap clustering of a transcript's ranges: backend.cluster_ranges_multiscale.

Backend.cluster_ranges embeds each range at ONE window length (wav.range_starts picks a bucket per range).  The eigengap clustering
(clustering="nmesc") was published together with multi-scale windows (Park et al., "Multi-scale speaker diarization with neural affinity
score fusion", ICASSP 2021) and NeMo's clustering diarizer runs it so: every stretch of speech is embedded at several window lengths, the
per-scale cosine affinities are mapped onto the shortest scale's windows and added with weights, and the eigengap search runs on that sum.
Long windows give stable speaker evidence, short ones the time resolution.

A function of a Backend and not a keyword of Backend.cluster_ranges: the Backend's public surface is pinned name for name and signature
for signature (tests/test_rules_cpu.py, tests/test_vbx_hmm_cpu.py), so the capability sits beside it, as backend.diarize_fused and the
other functions imported into backend.py do.  Backend.cluster_ranges itself is untouched.

Imports neither torch nor the library with the module (backend.py imports it, and that imports without torch)."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from .wav import scale_starts

DEFAULT_SCALES = (1.5, 1.0, 0.5)       # the three-scale setting the method's reference suggests, inside wav.BUCKETS_S; no weights are tuned here


def cluster_ranges_multiscale(be, samples: np.ndarray, ranges: List[Tuple[float, float]], scales=DEFAULT_SCALES, scale_weights=None, speakers=None,
                              clustering: str = "nmesc"):
    """Speaker labels for a transcript's single-speaker ranges from the fused affinity of several window lengths.
    scales: 1 .. 8 distinct members of wav.BUCKETS_S, used in descending order, the shortest being the BASE scale (wav.scale_starts states
    the windows, hop half the length, and the map).  scale_weights: None (equal), else one number per scale in descending order of length,
    finite, >= 0, not all zero, normalised to sum 1; no weights are tuned or learned here.  speakers: cluster.parse_speakers' bounds, part of
    the eigengap search.  clustering: "nmesc" only - the centroids of "ahc" and "vbx" have no fused form, and asking for them is a ValueError.
    The path: wav.scale_starts -> ONE be.embed_tables call (one upload, one forward sequence per scale) -> the scales' rows stacked in scale
    order with the maps offset to match -> cluster.nmesc_multiscale (sdk_knn_rows_fused, then the unchanged rule).
    Returns Backend.cluster_ranges' triple on the BASE windows: (labels [W] int32 per base window, windows [(range index, start s, end s)],
    range_labels [len(ranges)] int32: the majority label of a range's windows, ties to the smaller label, -1 for a range shorter than the
    base length).  One base window: label 0.  No base window: empty results.  A scale that no range can hold is a ValueError naming it.
    Not available with SDK_NO_TORCH=1, like cluster_ranges."""
    if be.lite:
        raise ValueError("cluster_ranges_multiscale needs the torch engine: not available with SDK_NO_TORCH=1")
    if clustering != "nmesc":
        raise ValueError(f"cluster_ranges_multiscale: scales need clustering=\"nmesc\" (the fused affinity has no form for {clustering!r})")
    import torch
    from .cluster import nmesc_multiscale, parse_speakers
    speakers = parse_speakers(speakers, "cluster_ranges_multiscale")
    rate = 16000                                                         # wav.range_starts' rate: the contract format
    starts_by, wins_by, maps, _ = scale_starts(len(samples), ranges, scales, rate)
    base = [(ri, x / rate, (x + L) / rate) for ri, x, L in wins_by[-1]]
    range_labels = np.full(len(ranges), -1, dtype=np.int32)
    if not base:
        return np.zeros(0, np.int32), [], range_labels
    if len(base) == 1:
        labels = np.zeros(1, np.int32)
    else:
        parts = be.embed_tables(samples, starts_by)
        lens = [w[0][2] for w in wins_by]                                # descending: the order of the maps' rows
        offs = np.concatenate([[0], np.cumsum([len(w) for w in wins_by])[:-1]]).astype(np.int32)
        E_all = torch.cat([parts[L][0] for L in lens]).contiguous()
        labels = nmesc_multiscale(be.engine(), E_all, maps + offs[:, None], scale_weights, speakers=speakers).labels
    per = {}
    for (ri, _, _), lab in zip(base, labels):
        per.setdefault(ri, []).append(int(lab))
    for ri, labs in per.items():
        range_labels[ri] = int(np.argmax(np.bincount(labs)))            # first maximum = the smaller label
    return labels, base, range_labels
