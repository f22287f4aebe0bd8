"""Speaker diarization - "who spoke when" for a recording with no transcript: the join of the PyanNet segmentation (segmentation.py), the
ResNet34 embedding (resnet.py) and the centroid-linkage clustering (cluster.agglomerative_cluster), as PyAnnote 3.1's pipeline joins them
("Pyannote local speaker diarization" in the upstream toolkit's backends.yaml).  The rules below are THIS build's statement, following
PyAnnote 3.1 as best known here; no checkpoint and no pyannote code is on hand, so PARITY IS UNPINNED, like the three stages joined, and the
tests pin these rules.

  chunks      10-s chunks at segmentation.chunk_starts (step_s apart, plus one ending at the recording's end), cut on the device
  decode      cls [C, F] uint8 = argmax powerset class per frame (ties to the lower class); activity and count come from cls alone
  masks       per (chunk, local speaker s): pooling weights over the T4 columns of the ResNet's last map.  Column j takes segmentation frame
              i(j) = min(F - 1, (j F) // T4); full[j] = s active at i(j); clean[j] = full[j] and count(i(j)) < 2; the weights are clean when
              sum clean >= MIN_CLEAN_COLUMNS, else full; valid = sum w >= MIN_VALID_COLUMNS (the unbiased variance needs two columns)
  embedding   one conv trunk per chunk, three masked statistics poolings on its last map (ResNet34.forward_masked), seg_1, L2 norm.
              PyAnnote embeds each (chunk, speaker) pair with a full forward on the same waveform; the mask enters at the pooling only, so
              sharing the trunk computes the same thing in a third of the work.
  training    rows that are valid and have TRAIN_CLEAN_DEN * clean_frames >= F go to cluster.agglomerative_cluster unchanged
  assignment  centroids = float64 mean of each cluster's training unit rows, re-normalised; every valid row with an active frame takes the
              centroid of largest cosine (ties to the lowest); every other pair gets -1.  No training row: one cluster of all valid active
              rows (centroid = their mean), or no speaker at all.
  constrained assignment (constrained=True; PyAnnote's constrained_argmax): same centroids, same candidates (the local speakers of a chunk
              with valid != 0 and active frames > 0, in slot order; every other pair gets -1 and its row is never read).  For a chunk with m
              candidates and K centroids: among all maps that give n = min(m, K) of the candidates pairwise different clusters and the
              other m - n candidates -1, the one with the largest total cosine, summed in slot order; ties to the lexicographically smallest
              label tuple in slot order, -1 ordered after every cluster.  Two local speakers of a chunk - two different people, says the
              segmentation - never share a cluster.  A candidate left without a cluster (K < m) is DROPPED, as in PyAnnote: when the
              clustering finds one speaker, overlapped speech of a second one is lost.  With K >= m the optimum uses, for every row, one
              of that row's m largest cosines (ties to the lower cluster), so at most 27 tuples are compared per chunk and no general
              Hungarian solver is needed.  Runs on the device (sdk_diarize_centroids, sdk_diarize_assign): the embeddings stay there.
  VBx         (clustering="vbx"; the clustering half of PyAnnote's speaker-diarization-community-1 pipeline, stated in cluster.vbx_cluster):
              the centroid linkage of the training rows, cut at `threshold` with no small-cluster fold, only INITIALISES a variational-Bayes
              mixture on the PLDA transform of those rows (plda.py); speakers that the cut over-split lose their weight and die out.  The
              kept speakers' centroids are the responsibility-weighted means of the original unit rows; every candidate row is then assigned
              by sdk_diarize_assign with the caller's `constrained` flag, so the stretch from embeddings to labels stays on the device and the
              result carries scores either way.  With fewer than two training rows: as "ahc" (one cluster or none).
  nmesc       (clustering="nmesc"; eigengap spectral clustering with normalised-maximum-eigengap pruning, NeMo's default, stated in cluster.py
              above NMESC_P_MAX; parity unpinned, the tests pin THIS rule): no threshold.  Each training row lists its 64 nearest rows by
              cosine (sdk_knn_rows); for every candidate p the graph pruned to p neighbours gives the lazy operator
              T_p = (I + D^-1/2 A_p D^-1/2) / 2, whose leading eigenvalues come from a subspace iteration on the device (from a dense host
              eigensolve at 64 rows or fewer); the largest eigengap of the candidate with the least p / gap is the speaker count, and the
              k-means of that candidate's Ritz vectors gives the labels.  `speakers` bounds the eigengap search itself, so `forced` stays
              None; `threshold` and `min_cluster_size` are not used and no small cluster is folded.  The labels go through
              sdk_diarize_centroids and sdk_diarize_assign with the caller's `constrained` flag, as VBx's centroids do, and the result
              carries scores and `nmesc` = {p, k, ps, eigenvalues, ratios}.  With fewer than two training rows: as "ahc" (one cluster or
              none).  nmesc: a dict of neighbours, max_count, n_iter, seed (cluster.nmesc_cluster's defaults otherwise).
  bounds      (speakers=; pyannote's num_speakers / min_speakers / max_speakers, written from the published description; parity unpinned, the
              tests pin THIS rule, stated in full in cluster.py above parse_speakers).  None: no bound, every result field is what it was.
              An int k >= 1: exactly k speakers; a pair (lo, hi), either side None, 1 <= lo <= hi: bounds; pyannote's max_speakers is
              speakers=(None, hi) here, while max_speakers below stays the cap PER FRAME and never touches the clustering.  The
              unbounded clustering runs first and finds K0 speakers ("ahc": the clusters after cut and fold; "vbx": the kept speakers).
              lo <= K0 <= hi: the result IS the unbounded one, bit for bit.  Otherwise target = lo when K0 < lo, else hi, clamped to
              1 .. N training rows.  "ahc": the level search of cluster.agglomerative_cluster rule 7 (host integers on Z, O(N)): the level
              whose count of clusters of the effective minimum size is nearest the target, then nearest the cut, then lowest, folded as
              the cut is; a target above K0 may be out of reach, then the closest count is taken.  "vbx": cluster.kmeans_cluster with
              k = target on the original unit rows of the training set (sdk_kmeans_rows: the whole loop in one enqueue), whose labels go
              through sdk_diarize_centroids and sdk_diarize_assign as VBx's centroids do; pi and elbo of the VBx pass that was overruled
              stay on the result.  With fewer than two training rows nothing is forced.  The result's `forced` is None, or
              {found: K0, target, method: "level" | "kmeans", level: t* or None, n_iter: int or None}.  In run_many the level search
              replaces the cut per recording inside _pack_ahc, on the host: the waits per pack do not grow.
  stitching   on the global frame grid of segmentation.aggregate_counts (frame g, centre 270 g + 495, takes frame g + q_c of chunk c,
              q_c = (135 - start_c) // 270): act[g, k] = chunks in which a local speaker labelled k is active; count[g] = the mean chunk count
              rounded half up, at most 2 and max_speakers; speakers[g] = the count[g] clusters of largest act > 0 (ties to the lower cluster)
  numbering   clusters are renumbered by first appearance in time: frame order, then slot order, of a provisional stitching pass (clusters
              that never surface keep their relative order behind the others); the stitching is then run with the final numbers
  turns       per speaker, runs of frames with segmentation.frames_to_ranges's boundaries; no gap filling unless asked for (smoothing,
              below); overlap gives simultaneous turns
  smoothing   (min_duration_off=, min_duration_on=; PyAnnote's Binarize hyper-parameters, in its order: fill, then drop) with either above 0
              the final speakers table is smoothed on the device before it comes down (smooth.py states the rule; csrc/smooth.hip): a
              speaker's pauses of at most min_duration_off are filled where the frame has a free slot under the cap per frame, then the
              runs shorter than min_duration_on are dropped; turns are cut from the smoothed table and the result's `smoothing` holds
              {min_duration_off, min_duration_on, fill, keep, filled, dropped}.  count, labels, centroids, scores, n_speakers and the
              numbering stay as they are.  In run_many the tallies ride in the download of the speakers table: the waits per pack do not
              grow.  Both at 0 (the default): the path is not entered and every result is what it was.  sweep(smoothing=[pairs]) scores
              every threshold under every pair; backend.smooth_diarization smooths finished results

  many        (Diarizer.run_many, Backend.diarize_many) a folder of recordings crosses the pipeline as packs: the recordings laid end to end in
              one buffer with CHUNK zero samples behind each (pack_recordings), so chunks of different recordings share the segmentation /
              embedding batches and a chunk that runs past its recording's end reads zeros, as it does alone; ONE grouped centroid_linkage
              launch for all recordings; the cut per recording on the host (integers and Z); fold, centroids, assignment, stitching and the
              renumbering by appearance in grouped kernels (sdk_diarize_*_grouped, sdk_diarize_first_seen, sdk_diarize_renumber) that find
              a chunk's, frame's or cluster's recording by binary search on prefix-sum tables.  The embeddings never leave the device and
              the host waits for the device a fixed number of times per pack.
  linking     (link_speakers, Backend.link_speakers) the speakers of many recordings as one inventory: the results' centroids, grouped by
              recording, go through the linked centroid linkage on the device (cluster.link_rows, sdk_linked_linkage: two speakers of one
              recording never join, merging stops at the threshold); enrolled profiles join as rows of one further group.  The rule is
              stated at link_speakers; run_many's results are not changed by it.
  streaming   (Diarizer.open_streams, Backend.open_streams) audio fed as it arrives, "who is speaking now" a bounded delay later: the same chunks
              and embed_chunks, then an inventory that grows online, the constrained assignment above against its centroids and a rolling
              stitch on this frame grid that emits frames once their latency has passed.  The rule, its numpy restatement and the bank of
              live streams that steps in one launch are stream.py's; run and run_many are not changed by it.
  score       (Diarizer.score, Backend.score_diarization) how good a result is: the diarization error rate of results against reference
              annotations (turn lists, or RTTM), on this frame grid.  The results' speakers tables are scored on the device as one pack -
              reference masks, co-occurrence tallies and the exact reference-to-hypothesis assignment in three integer kernels
              (csrc/score.hip).  The rule, its numpy restatement (score_host) and the RTTM reader are score.py's.  Opt-in, the DIHARD way
              (csrc/score_jer.hip): uem= scores only inside each recording's evaluation map (a UEM file, or interval lists), jer=True adds
              the Jaccard error rate - every reference speaker weighing the same - with purity and coverage; integers on the device, the
              same one download.
  sweep       (Diarizer.sweep, Backend.tune_diarization) the DER of run_many at many thresholds, for tuning the cut on a development set:
              per pack one embedding and one linkage (_pack_link), then per threshold the cut-to-centroids stage (_pack_cut), the grouped
              assignment and stitching, and the scoring kernels on the hypothesis where it lies; every threshold's tallies come down in one
              download per pack.  clustering="ahc" without speaker bounds only; run_many is not changed by it.  uem= and jer= as score's,
              without a further wait per pack; metric="jer" picks `best` by the pooled JER instead of the pooled DER.
  shared      run and run_many are one pipeline: Diarizer._check_options, _check_recording, _embed_all (the batches of embed_chunks) and
              _empty serve both, as do candidate_mask, training_mask and _speaker_cap; after the embedding run clusters one recording and
              run_many takes the pack through _pack_begin, _pack_vbx or _pack_ahc, _pack_assign and _pack_results.  They differ on purpose in
              two places, both for "ahc": run(constrained=False) assigns on the host (assign_rows, a BLAS product, no scores) and run folds
              small clusters on the host (cluster.agglomerative_cluster, a BLAS product), where run_many's grouped kernels sum every cosine
              in column order in float64 (every result carries scores).  So with constrained=True run_many's cls, info, labels, count,
              speakers, turns, n_speakers and starts equal run's, and with constrained=False too unless a decision is a tie or near-tie at
              float64 rounding; centroids agree to fp32 rounding of the same float64 rows.

Decode, masks, the constrained assignment and stitching run in libsdk_hip.so (csrc/diarize.hip), the pooling in csrc/resnet.hip; the *_host
functions of diarize_host.py restate them in numpy for hosts that post-process stored class tables.  The host receives info, the unit
embeddings (not with constrained=True: then labels, scores and centroids instead), and count / speakers only.
This module holds the rule and the Diarizer, and re-exports every name of diarize_host.py (constants, DiarizationResult, packing, the numpy
restatements), diarize_ops.py (the wrappers over sdk_diarize_*, GroupTables) and diarize_link.py (link_speakers).
"""
from __future__ import annotations

import os
import time
from dataclasses import dataclass
from typing import List, NamedTuple, Optional

import numpy as np

from .cluster import (KMEANS_HOST_READS, PYANNOTE_MIN_CLUSTER_SIZE, PYANNOTE_THRESHOLD, _flat_partition, agglomerative_cluster, cut_level,
                      effective_min_size, fcluster_distance, level_search, nmesc_cluster, parse_speakers, speaker_target, vbx_cluster)
from .diarize_host import (DEFAULT_BATCH, DEFAULT_PACK_LINKAGE_BYTES, DEFAULT_PACK_SAMPLES, MAX_ASSIGN_DIM, MAX_LINKAGE_ROWS, MAX_PACK_SAMPLES,  # noqa: F401
                           MIN_CLEAN_COLUMNS, MIN_VALID_COLUMNS, N_LOCAL, TRAIN_CLEAN_DEN, _COUNT, _MASK, DiarizationResult, Pack, _centroids64,
                           _dot_in_order, _speaker_cap, appearance_order, assign_constrained_host, assign_grouped_host, assign_rows, candidate_mask,
                           constrained_chunk, decode_host, first_seen_host, fold_grouped_host, global_frames, masks_host, pack_recordings, pack_rows,
                           reconstruct_grouped_host, reconstruct_host, reference_labels, renumber_host, split_packs, to_rttm, training_mask, training_rows, turns_from_frames)
from .diarize_link import SpeakerLinks, link_speakers, relabel_turns  # noqa: F401
from .diarize_ops import (LINKAGE_HOST_READS, VBX_HOST_READS, GroupTables, _check_dim, _check_rows, _check_tensor, _native, diarize_assign,  # noqa: F401
                          diarize_assign_grouped, diarize_centroids, diarize_first_seen, diarize_fold_grouped, diarize_masks, diarize_reconstruct,
                          diarize_reconstruct_grouped, diarize_renumber, powerset_decode)
from .segmentation import CHUNK, chunk_starts
from .segmentation import num_frames as seg_frames


def _nmesc_fields(nres) -> dict:
    """DiarizationResult.nmesc of a cluster.NmescResult."""
    return {"p": nres.p, "k": nres.n_speakers, "ps": nres.ps, "eigenvalues": nres.eigenvalues, "ratios": nres.ratios}


@dataclass(frozen=True)
class _Options:
    """The checked keywords of run, run_many and sweep, built once per call and handed down the stages."""
    step_s: float
    threshold: Optional[float]   # None in sweep, which hands _pack_cut each threshold of its own
    min_cluster_size: int
    max_speakers: Optional[int]
    constrained: bool
    clustering: str
    vbx: dict                    # _check_options' copy
    bounds: Optional[tuple]      # cluster.parse_speakers' result
    nmesc: Optional[dict] = None # _check_nmesc's copy
    smooth: Optional[tuple] = None   # (min_duration_off, min_duration_on, fill, keep) when either time is above 0 (_check_smoothing)


@dataclass
class _PackState:
    """One pack between its stages, as _pack_begin leaves it."""
    xs: list                     # the pack's recordings, int16 rows
    pack: Pack
    tab: GroupTables
    cls: object                  # [C, F] uint8 (device)
    info_dev: object             # [C, 3, 4] int32 (device)
    info: np.ndarray             # the same on the host
    E_dev: object                # [3 C, d] fp32 unit rows (device)
    rows: list                   # pack_rows: per recording, the rows that make its centroids
    n_train: list                # and how many of them are training rows
    sync: dict                   # the pack's entry of last_sync


class _Clusters(NamedTuple):
    """What a clustering stage (_pack_vbx, _pack_ahc, _pack_cut) hands to the assignment."""
    c32: object                  # [K, d] fp32 unit centroids of all recordings (device); None: no recording has a cluster
    c64: object                  # the same in float64, before the final rounding
    cent_off: np.ndarray         # [R + 1] int64 prefix sums of the recordings' cluster counts
    vres: dict                   # {recording: cluster.VbxResult}
    forced: dict                 # {recording: forced}
    nres: Optional[dict] = None  # {recording: cluster.NmescResult}


class Diarizer:
    """The pipeline on one ops.Engine: a resident segmentation.Segmentation and a resident embedding network - resnet.ResNet34, or
    ecapa_diar.EcapaEmbedder for a diarization in the ECAPA space; any object with .cfg.embed_dim, .precision, .last_map_frames(T) and
    .forward_masked(feats, B, T, w, valid) serves (the parameter and the attribute keep the name `resnet`; `embedder` is its read-only
    alias).  run and run_many share the option and recording checks, the embedding of all chunks (_embed_all) and the empty result; they
    part after that (the module docstring)."""

    def __init__(self, engine, segmentation, resnet, plda=None):
        self.eng, self.seg, self.resnet, self.plda = engine, segmentation, resnet, plda
        self.trace = False               # True: run_many appends one {stage: seconds} per pack to last_stage_s, every stage ended by a device synchronisation
        self.last_stage_s: List[dict] = []
        self.last_sync: List[dict] = []  # run_many: the downloads and uploads of the last call, one dict per pack

    @property
    def embedder(self):
        """The embedding network (read-only; the attribute `resnet` under its family-neutral name; the class docstring says what serves)."""
        return self.resnet

    def plda_model(self):
        """The plda.Plda of clustering="vbx": the one given, else a seeded synthetic model for the embedding width."""
        if self.plda is None:
            from .plda import synthetic_plda
            self.plda = synthetic_plda(self.resnet.cfg.embed_dim, 128, 0)
        return self.plda

    # ---------------------------------------------------------------------------------------------- what run and run_many share
    def _check_options(self, who: str, clustering, vbx, max_speakers, speakers=None):
        """-> (vbx as a dict of its own, the bounds of cluster.parse_speakers)."""
        if clustering not in ("ahc", "vbx", "nmesc"):
            raise ValueError(f"{who}: clustering={clustering!r} (\"ahc\", \"vbx\" or \"nmesc\")")
        vbx = dict(vbx or {})
        if set(vbx) - {"Fa", "Fb", "max_iters", "epsilon", "init_smoothing"} or (vbx and clustering != "vbx"):
            raise ValueError(f"{who}: vbx={vbx} (keys Fa, Fb, max_iters, epsilon, init_smoothing; only with clustering=\"vbx\")")
        if max_speakers is not None and int(max_speakers) < 0:
            raise ValueError(f"max_speakers={max_speakers}: must be None or >= 0")
        return vbx, parse_speakers(speakers, who)

    def _check_nmesc(self, who: str, clustering, nmesc) -> dict:
        """-> nmesc as a dict of its own."""
        nmesc = dict(nmesc or {})
        if set(nmesc) - {"neighbours", "max_count", "n_iter", "seed"} or (nmesc and clustering != "nmesc"):
            raise ValueError(f"{who}: nmesc={nmesc} (keys neighbours, max_count, n_iter, seed; only with clustering=\"nmesc\")")
        return nmesc

    def _check_smoothing(self, min_duration_off, min_duration_on) -> Optional[tuple]:
        """-> None when both times are 0 (the path is not entered), else (min_duration_off, min_duration_on, fill, keep)."""
        from .smooth import fill_frames_of, keep_frames_of
        fill, keep = fill_frames_of(min_duration_off), keep_frames_of(min_duration_on)
        return (float(min_duration_off), float(min_duration_on), fill, keep) if float(min_duration_off) > 0.0 or float(min_duration_on) > 0.0 else None

    def _smoothed(self, res: DiarizationResult, smooth: Optional[tuple], tally=(0, 0)) -> DiarizationResult:
        if smooth is not None:
            from .smooth import smoothing_fields
            res.smoothing = smoothing_fields(*smooth, tally)
        return res

    def _check_recording(self, who: str, n_samples: int, step_s: float, logp=None) -> int:
        """The linkage's row bound and the shape of an injected logp, for a recording of n_samples > 0 samples -> its number of chunks."""
        Cn, F = len(chunk_starts(n_samples, step_s)), seg_frames(CHUNK)
        if N_LOCAL * Cn > MAX_LINKAGE_ROWS:
            raise ValueError(f"{who}: {Cn} chunks at step_s={step_s} give up to {N_LOCAL * Cn} embeddings to cluster; the centroid linkage serves at "
                             f"most {MAX_LINKAGE_ROWS} rows ({MAX_LINKAGE_ROWS // N_LOCAL} chunks): raise step_s or split the recording")
        if logp is not None:
            shp = tuple(logp.shape if hasattr(logp, "shape") else np.shape(logp))
            if shp != (Cn, F, 7):
                raise ValueError(f"{who}: injected logp must be [{Cn}, {F}, 7] for {n_samples} samples at step_s={step_s}, got {shp}")
        return Cn

    def _empty(self) -> DiarizationResult:
        d = self.resnet.cfg.embed_dim
        return DiarizationResult([], 0, np.zeros((0, d), np.float32), np.zeros((0, N_LOCAL), np.int32), np.zeros(0, np.uint8),
                                 np.full((0, 2), -1, np.int32), np.zeros(0, np.int64), np.zeros((0, N_LOCAL, 4), np.int32))

    def embed_chunks(self, rec, n_samples: int, starts_dev, logp=None):
        """One batch of chunks: (cls [B, F] uint8, info [B, 3, 4] int32, unit embeddings [B * 3, d] fp32), all on the device."""
        from .ops import num_frames as fbank_frames
        B = int(starts_dev.numel())
        lp = logp if logp is not None else self.seg.forward(rec, starts_dev)
        cls = powerset_decode(self.eng, lp)
        T = fbank_frames(CHUNK)
        w, info = diarize_masks(self.eng, cls, self.resnet.last_map_frames(T))
        feats = self.eng.fbank_windows(rec.data_ptr(), n_samples, starts_dev.data_ptr(), B, CHUNK)
        emb = self.resnet.forward_masked(feats, B, T, w, info[:, :, 3].contiguous())
        return cls, info, self.eng.l2norm(emb)[0]

    def _embed_all(self, rec, n: int, starts_dev, logp_dev=None):
        """Every chunk of the buffer rec (n samples, device) in batches of $SDK_DIARIZE_BATCH -> (cls [C, F] uint8, info [C, 3, 4] int32,
        unit embeddings [3 C, d] fp32) on the device.  In a pack the batches cross recording boundaries."""
        torch = _native()[0]
        Cn = int(starts_dev.numel())
        batch = max(1, int(os.environ.get("SDK_DIARIZE_BATCH", str(DEFAULT_BATCH))))
        cls = torch.empty((Cn, seg_frames(CHUNK)), dtype=torch.uint8, device=self.eng.device)
        infos, embs = [], []
        for a in range(0, Cn, batch):
            c, i, e = self.embed_chunks(rec, n, starts_dev[a:a + batch], None if logp_dev is None else logp_dev[a:a + batch])
            cls[a:a + batch] = c
            infos.append(i)
            embs.append(e)
        return cls, torch.cat(infos), torch.cat(embs)

    def open_streams(self, n_streams: int = 1, **options):
        """A stream.StreamBank of n_streams live streams on this pipeline (options: step_s, latency_s, capacity, delta_new, max_speakers;
        stream.py states the rule)."""
        from .stream import StreamBank
        return StreamBank(self, n_streams, **options)

    # ---------------------------------------------------------------------------------------------- one recording
    def run(self, samples, step_s: float = 1.0, threshold: float = PYANNOTE_THRESHOLD, min_cluster_size: int = PYANNOTE_MIN_CLUSTER_SIZE,
            max_speakers: Optional[int] = None, logp=None, constrained: bool = False, clustering: str = "ahc",
            vbx: Optional[dict] = None, speakers=None, nmesc: Optional[dict] = None, min_duration_off: float = 0.0,
            min_duration_on: float = 0.0) -> DiarizationResult:
        """samples: 16 kHz mono int16 (host) -> DiarizationResult.  logp [C, 589, 7] (fp32, host or device) replaces the segmentation
        model's output (the chunks are chunk_starts(len(samples), step_s)).  The default threshold and size are PyAnnote 3.1's, tuned for
        ITS trained embedding; with other weights pass a threshold of your own.  constrained=True: the constrained assignment of the
        module docstring, on the device (the result carries scores); False: every row takes its nearest centroid on its own.
        clustering="vbx": the VBx clustering of the module docstring instead of the cut-and-fold ("ahc", the default); `threshold` keeps its
        meaning, the cut of the linkage, which now only initialises: pass cluster.VBX_AHC_THRESHOLD (0.6) with it; min_cluster_size is not
        used.  vbx: a dict of Fa, Fb, max_iters, epsilon, init_smoothing (cluster.vbx_cluster's defaults otherwise).  The result carries
        scores, pi and elbo.
        clustering="nmesc": the eigengap spectral clustering of the module docstring (cluster.nmesc_cluster): threshold and min_cluster_size
        are not used; nmesc: a dict of neighbours, max_count, n_iter, seed.  The result carries scores and `nmesc`; `speakers` bounds the
        eigengap search and `forced` stays None.
        speakers: the number of speakers of the recording, "bounds" in the module docstring: None, an int k (exactly k) or a pair (lo, hi),
        either side None.  pyannote's num_speakers=k is speakers=k, its min_speakers / max_speakers are speakers=(lo, hi), its
        max_speakers alone is speakers=(None, hi); max_speakers HERE is the cap per frame and keeps that meaning.  The result's `forced`
        says whether the clustering was overruled.
        min_duration_off, min_duration_on: seconds, "smoothing" in the module docstring - a speaker's pauses no longer than the first are
        filled, then the turns shorter than the second are dropped, on the device; the result's `smoothing` says what was done."""
        vbx, bounds = self._check_options("diarize", clustering, vbx, max_speakers, speakers)
        nmesc = self._check_nmesc("diarize", clustering, nmesc)
        smooth = self._check_smoothing(min_duration_off, min_duration_on)
        torch, eng = _native()[0], self.eng
        x = np.ascontiguousarray(samples, dtype=np.int16).reshape(-1)
        if x.size == 0:
            return self._smoothed(self._empty(), smooth)
        st = chunk_starts(x.size, step_s)                       # chunks
        Cn, F = self._check_recording("diarize", x.size, step_s, logp), seg_frames(CHUNK)
        if logp is not None:
            logp = torch.as_tensor(logp, dtype=torch.float32).to(eng.device)
        if eng.precision != self.resnet.precision:
            eng.set_precision(self.resnet.precision)            # the front end's output format follows the embedding's numerical contract
        rec = torch.from_numpy(x).to(eng.device)
        starts_dev = torch.from_numpy(st.astype(np.int32)).to(eng.device)
        cls, info_dev, E_dev = self._embed_all(rec, x.size, starts_dev, logp)     # decode, masks, embedding
        info = info_dev.cpu().numpy()
        train = training_rows(info, F)                          # training rows and their clustering
        vres, nres, tl, forced = None, None, np.zeros(len(train), np.int32), None
        if len(train) > 1 and clustering == "nmesc":
            nres = nmesc_cluster(eng, E_dev, rows=train, speakers=bounds, **nmesc)
            tl = nres.labels
        elif len(train) > 1 and clustering == "vbx":
            vres = vbx_cluster(eng, E_dev, self.plda_model(), threshold, rows=train, speakers=bounds, **vbx)
            forced = vres.forced
        elif len(train) > 1:
            ares = agglomerative_cluster(eng, E_dev.index_select(0, torch.from_numpy(train).to(eng.device)).contiguous(), threshold, min_cluster_size,
                                         speakers=bounds)
            tl, forced = ares.labels, ares.forced
        if constrained or clustering != "ahc":                  # assignment on the device: the embeddings stay there, the result carries scores
            if vres is not None:
                c32, c64 = vres.cent, vres.cent64.contiguous()
            else:
                rows = train if len(train) else np.flatnonzero(candidate_mask(info))                 # no training row: the candidates, one cluster
                rl = np.asarray(tl, dtype=np.int32) if len(train) else np.zeros(len(rows), np.int32)
                c32, c64 = diarize_centroids(eng, E_dev, torch.from_numpy(rows.astype(np.int32)).to(eng.device), torch.from_numpy(rl).to(eng.device),
                                             int(rl.max()) + 1) if len(rows) else (None, None)
            if c64 is not None:
                lab_dev, score_dev = diarize_assign(eng, E_dev, info_dev, c64, bool(constrained))
                labels, scores, cent = lab_dev.cpu().numpy(), score_dev.cpu().numpy(), c32.cpu().numpy()
            else:                                               # neither a training row nor a candidate: no speaker
                labels, scores, cent = np.full((Cn, N_LOCAL), -1, np.int32), np.zeros((Cn, N_LOCAL), np.float32), np.zeros((0, self.resnet.cfg.embed_dim), np.float32)
        else:                                                   # assignment of "ahc" unconstrained: on the host, a BLAS product (the module docstring)
            E = E_dev.cpu().numpy()
            E[info.reshape(-1, 4)[:, 3] == 0] = 0.0            # rows that are not valid are never read as embeddings
            labels, cent = assign_rows(E, info, train, tl)
            scores = None
        K, last = cent.shape[0], {}

        def stitch(lab):                                        # stitching; numbering by appearance below, then turns
            cnt, spk, _ = diarize_reconstruct(eng, cls, starts_dev, torch.from_numpy(np.ascontiguousarray(lab, dtype=np.int32)).to(eng.device),
                                              max(K, 1), x.size, max_speakers)
            last["spk_dev"] = spk                               # the table where it lies, for the smoothing below
            return cnt.cpu().numpy(), spk.cpu().numpy()
        count, speakers = stitch(labels)
        if K > 1:
            new = appearance_order(speakers, K)
            if not np.array_equal(new, np.arange(K)):
                labels = np.where(labels >= 0, new[np.maximum(labels, 0)], -1).astype(np.int32)
                cent = cent[np.argsort(new)]
                count, speakers = stitch(labels)
        tally = (0, 0)
        if smooth is not None:                                  # fill, then drop, on the table where it lies; one download with the tallies
            from .smooth import smooth_turns
            off = torch.tensor([0, len(speakers), 0, K], dtype=torch.int32).to(eng.device)
            spk_dev, tal_dev = smooth_turns(eng, last["spk_dev"], (off[:2], off[2:]), smooth[2], smooth[3], max(_speaker_cap(max_speakers), 1))
            flat = torch.cat([spk_dev.reshape(-1), tal_dev.reshape(-1)]).cpu().numpy()
            speakers, tally = flat[:-2].reshape(-1, 2).copy(), flat[-2:]
        res = self._smoothed(DiarizationResult(turns_from_frames(speakers, K), K, cent, labels, count, speakers, st, info, cls, scores), smooth, tally)
        if vres is not None:
            res.pi, res.elbo = vres.pi, vres.elbo
        if nres is not None:
            res.nmesc = _nmesc_fields(nres)
        if forced is not None:
            res.forced = forced
        return res

    # ---------------------------------------------------------------------------------------------- many recordings in one device pass
    def run_many(self, recordings, step_s: float = 1.0, threshold: float = PYANNOTE_THRESHOLD, min_cluster_size: int = PYANNOTE_MIN_CLUSTER_SIZE,
                 max_speakers: Optional[int] = None, logp=None, constrained: bool = False, clustering: str = "ahc",
                 vbx: Optional[dict] = None, speakers=None, nmesc: Optional[dict] = None, min_duration_off: float = 0.0,
                 min_duration_on: float = 0.0) -> List[DiarizationResult]:
        """recordings: a list of 16 kHz mono int16 arrays (host) -> one DiarizationResult per recording, in order; the keywords are run's,
        logp is None or a list with one [C_r, 589, 7] array per recording.  The recordings cross the pipeline in packs (pack_recordings) of
        at most $SDK_DIARIZE_PACK_SAMPLES samples (default 2^28, gaps included) whose grouped linkage stays within
        $SDK_DIARIZE_PACK_LINKAGE_BYTES of distance matrices (default 2^34; Engine.centroid_linkage serves any number of problems of at
        most 65 536 rows each); a recording that exceeds either bound alone is a pack of its own.  Per pack: one upload, the batches of
        $SDK_DIARIZE_BATCH chunks (they cross recording boundaries), one download of info, one grouped linkage launch over the recordings
        with at least two training rows and the download of its status and Z, the cut per recording on the host, then centroids of the cut,
        fold, final centroids, assignment, stitching, renumbering and second stitching on the device, and one download each of labels,
        scores, centroids, count and speakers.  self.last_sync holds the number of such waits of the last call, per pack.
        Where the results differ from run's on purpose: "shared" in the module docstring.  clustering="vbx" runs cluster.vbx_cluster
        recording by recording (its own linkage, cut and host reads) between the packed embedding and the grouped assignment.
        speakers: run's, applied to every recording; for "ahc" the level search replaces the cut on the host and adds no wait, for "vbx" a
        recording whose count is overruled adds cluster.KMEANS_HOST_READS waits.  clustering="nmesc" runs cluster.nmesc_cluster recording
        by recording in the same place (_pack_nmesc), as "vbx" does; its waits per recording (NmescResult.host_reads: the status of the
        lists, the eigenvalue table or the lists, the labels) are counted in last_sync.
        min_duration_off, min_duration_on: run's; the pack's speakers table is smoothed on the device after the second stitching
        (sdk_smooth_turns) and its tallies ride in the table's download, so last_sync is what it is without them."""
        vbx, bounds = self._check_options("diarize_many", clustering, vbx, max_speakers, speakers)
        opts = _Options(step_s, threshold, min_cluster_size, max_speakers, bool(constrained), clustering, vbx, bounds,
                        self._check_nmesc("diarize_many", clustering, nmesc), self._check_smoothing(min_duration_off, min_duration_on))
        xs, packs = self._plan_packs(recordings, logp, step_s)
        out: List[Optional[DiarizationResult]] = [None] * len(xs)
        self.last_sync = []
        for idx in packs:
            for i, res in zip(idx, self._run_pack([xs[i] for i in idx], None if logp is None else [logp[i] for i in idx], opts)):
                out[i] = res
        return out

    def _plan_packs(self, recordings, logp, step_s):
        """run_many's and sweep's checks of the recordings and their split into packs -> (xs as int16 rows, [[recording index]] per pack)."""
        xs = [np.ascontiguousarray(x, dtype=np.int16).reshape(-1) for x in recordings]
        if logp is not None and (not isinstance(logp, (list, tuple)) or len(logp) != len(xs)):
            raise ValueError(f"diarize_many: logp must be None or a list with one array per recording ({len(xs)}), got "
                             f"{len(logp) if isinstance(logp, (list, tuple)) else type(logp).__name__}")
        n_chunks = [self._check_recording(f"diarize_many: recording {i}", x.size, step_s, None if logp is None else logp[i]) if x.size else 0
                    for i, x in enumerate(xs)]
        return xs, split_packs([x.size for x in xs], n_chunks)

    # ---------------------------------------------------------------------------------------------- scoring against a reference, threshold sweep
    def score(self, results, references, collar_s: float = 0.0, skip_overlap: bool = False, uem=None, jer: bool = False, uris=None):
        """DiarizationResults (run's, run_many's or a finished stream's) and one reference turn list [(start_s, end_s, name)] per result ->
        one score.DerResult per result: their `speakers` are uploaded and scored on the device as one pack (score.py states the rule).
        uem: one entry per result (None, or the [(start_s, end_s)] outside which nothing is scored), or a UEM path or text with `uris` naming
        the results' recordings in it.  jer=True: the Jaccard error rate, purity and coverage too (the result's fields from jer on)."""
        from .score import resolve_uems, score_results
        results = list(results)
        return score_results(self.eng, results, references, collar_s, skip_overlap, resolve_uems("score", uem, uris, len(results)), jer)

    def sweep(self, recordings, references, thresholds, step_s: float = 1.0, min_cluster_size: int = PYANNOTE_MIN_CLUSTER_SIZE,
              max_speakers: Optional[int] = None, logp=None, constrained: bool = False, collar_s: float = 0.0, skip_overlap: bool = False,
              clustering: str = "ahc", speakers=None, uem=None, jer: bool = False, metric: str = "der", uris=None, smoothing=None):
        """The DER of run_many(recordings, threshold=t, ...) against `references` for every t of `thresholds` -> score.SweepResult
        (thresholds, per_recording [T][R], pooled [T], best).  Per pack the recordings are embedded ONCE and linked ONCE (_pack_embed,
        _pack_link); per threshold only the cheap tail runs - cut on host integers, fold, centroids, assignment, stitching, renumbering and
        second stitching exactly as run_many's (_pack_cut, _pack_assign_dev), then the three scoring kernels on the hypothesis where it
        lies.  The tallies of all thresholds stay on the device and come down in one download per pack: the waits per pack (last_sync) do
        not grow with the number of thresholds.  Only clustering="ahc" without speaker bounds: the sweep is over the cut of the linkage.
        A recording that the cut splits into more than score.MAX_SCORE_SPEAKERS speakers at some threshold is a ValueError.
        uem, jer, uris: as score's; the UEM intervals ride in the reference's upload and the Jaccard tables in the one download, so the waits
        per pack stay what they are.  metric: "der" or "jer" (which computes the JER whatever jer says) - what `best` minimises.
        smoothing: None (this call as it always was), or a list of (min_duration_off, min_duration_on) pairs ("smoothing" in the module
        docstring): per threshold the tail still runs once, and per pair sdk_smooth_turns and the scoring kernels run on the smoothed table
        where it lies (the pair (0, 0) scores the table as it is); everything comes down in the same one download per pack, and last_sync
        is what it is without the keyword.  -> score.SmoothSweepResult (thresholds, smoothing, per_recording [T][S][R], pooled [T][S],
        best = (threshold, min_duration_off, min_duration_on): the least pooled metric, ties across thresholds as SweepResult.best breaks
        them, then to the earlier pair)."""
        from .smooth import check_pairs, smooth_turns
        from .score import SmoothSweepResult, SweepResult, best_threshold, check_metric, pool, rasterise_references, resolve_uems, score_host, score_tables
        jer = bool(jer) or check_metric("sweep", metric) == "jer"
        if clustering != "ahc" or speakers is not None:
            raise ValueError(f"sweep: clustering={clustering!r}, speakers={speakers!r}: the sweep is over the cut of clustering=\"ahc\" with speakers=None")
        vbx, bounds = self._check_options("sweep", clustering, None, max_speakers, None)
        opts = _Options(step_s, None, min_cluster_size, max_speakers, bool(constrained), clustering, vbx, bounds)
        ths = [float(t) for t in thresholds]
        if not ths or any(t != t for t in ths):
            raise ValueError(f"sweep: thresholds={list(thresholds)!r} (at least one number)")
        references = list(references)
        if len(references) != len(recordings):
            raise ValueError(f"sweep: {len(references)} references for {len(recordings)} recordings")
        uems = resolve_uems("sweep", uem, uris, len(recordings))
        pairs = check_pairs("sweep", smoothing)
        cols = [None] if pairs is None else pairs               # what every threshold's table is scored under; None: as it is
        cap = max(_speaker_cap(max_speakers), 1)
        xs, packs = self._plan_packs(recordings, logp, step_s)
        per = [[[None] * len(xs) for _ in cols] for _ in ths]   # [T][S][R]
        self.last_sync = []
        for idx in packs:
            refs, pack_uems = [references[i] for i in idx], None if uems is None else [uems[i] for i in idx]
            p = self._pack_begin([xs[i] for i in idx], None if logp is None else [logp[i] for i in idx], opts)
            if p is None:                                         # nothing but empty recordings: no frame to score
                for t in range(len(ths)):
                    for s in range(len(cols)):
                        for k, (i, ref) in enumerate(zip(idx, refs)):
                            per[t][s][i] = score_host(np.zeros((0, 2), np.int32), 0, ref, collar_s, skip_overlap, None if uems is None else pack_uems[k], jer)
                continue
            torch, tab = _native()[0], p.tab
            linkage = self._pack_link(p)
            ref = rasterise_references(self.eng, tab, refs, collar_s, skip_overlap, upload=self._up, uems=pack_uems)
            self._mark("reference")
            held, pieces = [], []                                 # one score.ScoreTables per (threshold, pair) and the int64 pieces of them all
            for t in ths:
                cl = self._pack_cut(p, linkage, t, opts)
                tab.set_clusters(cl.cent_off)
                self._mark("cut_fold_centroids")
                spk_dev = self._pack_assign_dev(p, cl, opts)[4]
                self._mark("assign_stitch")
                co_off_d = []                                     # the threshold's co_off goes up once, whatever the number of pairs

                def up_once(a):
                    if not co_off_d:
                        co_off_d.append(self._up(a))
                    return co_off_d[0]
                for pair in cols:
                    hyp = spk_dev if pair is None or (pair[2] == 0 and pair[3] == 0) else smooth_turns(self.eng, spk_dev, tab, pair[2], pair[3], cap)[0]
                    held.append(score_tables(self.eng, hyp, tab, ref, upload=up_once, jer=jer))
                    pieces += held[-1].pieces()
                self._mark("score")
            p.sync["uploads"] += tab.uploads
            flat = self._down(torch.cat(pieces))                  # every threshold's tallies, tables and maps: ONE download
            pos = 0
            for n_col, tables in enumerate(held):
                t, s = divmod(n_col, len(cols))
                for i, one in zip(idx, tables.results(ref, flat[pos:pos + tables.size])):
                    per[t][s][i] = one
                pos += tables.size
            self._mark("download")
        if pairs is None:
            per = [row[0] for row in per]
            pooled = [pool(row) for row in per]
            return SweepResult(ths, per, pooled, best_threshold(ths, pooled, metric))
        pooled = [[pool(row) for row in per_t] for per_t in per]
        t, s = min(((t, s) for t in range(len(ths)) for s in range(len(cols))),
                   key=lambda ts: (getattr(pooled[ts[0]][ts[1]], metric), abs(ths[ts[0]] - PYANNOTE_THRESHOLD), ths[ts[0]], ts[1]))
        return SmoothSweepResult(ths, [(a, b) for a, b, _, _ in pairs], per, pooled, (ths[t], pairs[s][0], pairs[s][1]))

    # ---------------------------------------------------------------------------------------------- labelled rows for training a PLDA
    def plda_rows(self, samples_list, references, step_s: float = 1.0, logp=None) -> dict:
        """The training rows of the recordings with the reference speaker each belongs to, for plda.fit (Backend.train_plda).  references:
        one turn list [(start_s, end_s, name)] per recording; logp as run_many's.  The recordings go through _embed_all in packs, as
        run_many's do, and the embeddings stay on the device; per pack the class tables come down once and every training row
        (training_mask) is labelled on the host in integers (diarize_host.reference_labels states the rule; the reference is
        score.prepare_reference rasterised by score.reference_masks_host, no collar).  -> dict(E [n, d] fp32 unit rows on the device, the
        labelled rows in recording then row order; recording [n], row [n] (c * 3 + s inside the recording) and speaker [n] int32 (the index
        into names[recording]); names: one list per recording; n_training, n_dropped: the training rows seen and those left out)."""
        from .score import MAX_SCORE_SPEAKERS, prepare_reference, reference_masks_host
        torch = _native()[0]
        references = list(references)
        if len(references) != len(samples_list):
            raise ValueError(f"plda_rows: {len(references)} references for {len(samples_list)} recordings")
        opts = _Options(step_s, None, PYANNOTE_MIN_CLUSTER_SIZE, None, False, "ahc", {}, None)
        xs, packs = self._plan_packs(samples_list, logp, step_s)
        names: List[list] = [[] for _ in xs]
        E, rec_of, row_of, spk_of = [], [], [], []
        n_training = 0
        self.last_sync = []
        for idx in packs:
            p = self._pack_begin([xs[i] for i in idx], None if logp is None else [logp[i] for i in idx], opts)
            if p is None:
                continue
            cls = self._down(p.cls)
            co, fo = p.pack.chunk_off, p.pack.frame_off
            take = []
            for r, i in enumerate(idx):
                merged, names[i] = prepare_reference(references[i])
                if len(names[i]) > MAX_SCORE_SPEAKERS:
                    raise ValueError(f"plda_rows: recording {i} has {len(names[i])} reference speakers; at most {MAX_SCORE_SPEAKERS}")
                a, b = int(co[r]), int(co[r + 1])
                mask, _ = reference_masks_host(merged, int(fo[r + 1] - fo[r]))
                lab = reference_labels(cls[a:b], p.info[a:b], p.pack.starts_local[a:b], mask, len(names[i]))
                n_training += int(training_mask(p.info[a:b], cls.shape[1]).sum())
                rows = np.flatnonzero(lab >= 0)
                take.append(N_LOCAL * a + rows)
                rec_of.append(np.full(len(rows), i, np.int32))
                row_of.append(rows.astype(np.int32))
                spk_of.append(lab[rows])
            take = np.concatenate(take)
            if len(take):
                E.append(p.E_dev.index_select(0, self._up(take.astype(np.int64))))
        cat = (lambda v: np.concatenate(v) if v else np.zeros(0, np.int32))
        d = self.resnet.cfg.embed_dim
        E_all = torch.cat(E).contiguous() if E else torch.empty((0, d), dtype=torch.float32, device=self.eng.device)
        return dict(E=E_all, recording=cat(rec_of), row=cat(row_of), speaker=cat(spk_of), names=names, n_training=n_training,
                    n_dropped=n_training - int(E_all.shape[0]))

    def _up(self, a, dtype=None):                              # host -> device, counted for the current pack (dtype: torch.as_tensor converts on the way)
        torch = _native()[0]
        self.last_sync[-1]["uploads"] += 1
        return (torch.from_numpy(np.ascontiguousarray(a)) if dtype is None else torch.as_tensor(a, dtype=dtype)).to(self.eng.device)

    def _down(self, t) -> np.ndarray:                           # device -> host, a wait for the device, counted for the current pack
        self.last_sync[-1]["downloads"] += 1
        return t.cpu().numpy()

    def _mark(self, name: str):
        """self.trace: the wall clock since the last mark goes to stage `name` of the current pack, after a device synchronisation."""
        if self.trace:
            _native()[0].cuda.synchronize()
            now, stage_s = time.perf_counter(), self.last_stage_s[-1]
            stage_s[name] = stage_s.get(name, 0.0) + now - self._t_mark
            self._t_mark = now

    def _run_pack(self, xs, logps, opts: _Options):
        """One pack through its stages; every _mark ends a stage of last_stage_s."""
        p = self._pack_begin(xs, logps, opts)
        if p is None:
            return [self._smoothed(self._empty(), opts.smooth) for _ in xs]
        cl = {"vbx": self._pack_vbx, "nmesc": self._pack_nmesc}.get(opts.clustering, self._pack_ahc)(p, opts)
        p.tab.set_clusters(cl.cent_off)
        p.sync["uploads"] += p.tab.uploads
        self._mark("cut_fold_centroids")
        host = self._pack_assign(p, cl, opts)
        self._mark("assign_stitch_download")
        out = self._pack_results(p, cl, host, opts.smooth)
        self._mark("turns")
        return out

    def _pack_begin(self, xs, logps, opts: _Options) -> Optional[_PackState]:
        """What run_many and sweep do first with a pack: its entry of last_sync (and of last_stage_s), the packing, the upload and the
        embedding, the download of info and the rows that make the centroids -> _PackState; None when the pack has no chunk."""
        sync = {"downloads": 0, "uploads": 0}
        self.last_sync.append(sync)
        if self.trace:
            self.last_stage_s.append({})
        self._t_mark = time.perf_counter()
        pack = pack_recordings(xs, opts.step_s)
        if int(pack.chunk_off[-1]) == 0:
            return None
        tab, cls, info_dev, E_dev = self._pack_embed(pack, xs, logps)
        info = self._down(info_dev)
        self._mark("segmentation_embedding")
        rows, n_train = pack_rows(info, pack.chunk_off)
        return _PackState(xs, pack, tab, cls, info_dev, info, E_dev, rows, n_train, sync)

    def _pack_embed(self, pack: Pack, xs, logps):
        """Upload the pack and its tables, then embed every chunk -> (tab, cls, info_dev, E_dev)."""
        torch = _native()[0]
        if self.eng.precision != self.resnet.precision:
            self.eng.set_precision(self.resnet.precision)       # the front end's output format follows the embedding's numerical contract
        rec = self._up(pack.samples)
        starts_dev = self._up(pack.starts_packed)
        tab = GroupTables(self.eng, pack.chunk_off, pack.frame_off, pack.n_samples, pack.starts_local)
        lp_all = None
        if logps is not None:
            lp_all = torch.cat([self._up(l, torch.float32) for l, x in zip(logps, xs) if x.size])
        self._mark("pack_upload")
        return (tab,) + self._embed_all(rec, int(rec.numel()), starts_dev, lp_all)

    def _pack_vbx(self, p: _PackState, opts: _Options) -> _Clusters:
        """cluster.vbx_cluster recording by recording (its own linkage, cut and host reads)."""
        torch = _native()[0]
        E_dev, co, rows = p.E_dev, p.pack.chunk_off, p.rows
        vres, cents, K_r, forced = {}, [], [], {}
        for r in range(len(rows)):
            a, K = N_LOCAL * int(co[r]), min(len(rows[r]), 1)
            if p.n_train[r] > 1:
                v = vres[r] = vbx_cluster(self.eng, E_dev[a:N_LOCAL * int(co[r + 1])], self.plda_model(), opts.threshold, rows=rows[r] - a,
                                          speakers=opts.bounds, **opts.vbx)
                p.sync["downloads"] += VBX_HOST_READS
                if v.forced is not None:
                    forced[r] = v.forced
                    p.sync["downloads"] += KMEANS_HOST_READS
                cents.append((v.cent, v.cent64))
                K = int(v.n_speakers)
            elif K:                                             # one training row, or the candidates: one cluster
                cents.append(diarize_centroids(self.eng, E_dev, self._up(rows[r].astype(np.int32)),
                                               torch.zeros(len(rows[r]), dtype=torch.int32, device=self.eng.device), 1, check_rows=False))
            K_r.append(K)
        c32, c64 = (torch.cat(c).contiguous() for c in zip(*cents)) if cents else (None, None)    # None: no recording has a cluster
        return _Clusters(c32, c64, np.concatenate([[0], np.cumsum(K_r)]).astype(np.int64), vres, forced)

    def _pack_nmesc(self, p: _PackState, opts: _Options) -> _Clusters:
        """cluster.nmesc_cluster recording by recording, as _pack_vbx runs VBx: between the packed embedding and the grouped assignment.  A
        recording's labels go through sdk_diarize_centroids; its host reads (NmescResult.host_reads) are counted in last_sync."""
        torch = _native()[0]
        E_dev, co, rows = p.E_dev, p.pack.chunk_off, p.rows
        nres, cents, K_r = {}, [], []
        for r in range(len(rows)):
            a, K = N_LOCAL * int(co[r]), min(len(rows[r]), 1)
            lab = np.zeros(len(rows[r]), np.int32)                # one training row, or the candidates: one cluster
            if p.n_train[r] > 1:
                v = nres[r] = nmesc_cluster(self.eng, E_dev[a:N_LOCAL * int(co[r + 1])], rows=rows[r] - a, speakers=opts.bounds, **opts.nmesc)
                p.sync["downloads"] += v.host_reads
                lab, K = v.labels, int(v.n_speakers)
            if K:
                cents.append(diarize_centroids(self.eng, E_dev, self._up(rows[r].astype(np.int32)), self._up(lab.astype(np.int32)), K, check_rows=False))
            K_r.append(K)
        c32, c64 = (torch.cat(c).contiguous() for c in zip(*cents)) if cents else (None, None)    # None: no recording has a cluster
        return _Clusters(c32, c64, np.concatenate([[0], np.cumsum(K_r)]).astype(np.int64), {}, {}, nres)

    def _pack_ahc(self, p: _PackState, opts: _Options) -> _Clusters:
        """The linkage stage (_pack_link), then the cut-to-centroids stage (_pack_cut)."""
        return self._pack_cut(p, self._pack_link(p), opts.threshold, opts)

    def _pack_link(self, p: _PackState):
        """ONE grouped linkage over the recordings with at least two training rows -> (those recordings, the prefix sums of their training
        rows, Z on the host); (no recording, None, None) when there is nothing to link.  It does not depend on the threshold: sweep runs it
        once per pack."""
        link = [r for r in range(len(p.rows)) if p.n_train[r] > 1]
        if not link:
            return link, None, None
        off = np.concatenate([[0], np.cumsum([p.n_train[r] for r in link])]).astype(np.int64)
        E_link = p.E_dev.index_select(0, self._up(np.concatenate([p.rows[r] for r in link]))).contiguous()
        Z = self._down(self.eng.centroid_linkage(E_link, off))                     # ONE launch for all recordings; reads status, then Z
        p.sync["downloads"] += LINKAGE_HOST_READS
        self._mark("linkage")
        return link, off, Z

    def _pack_cut(self, p: _PackState, linkage, threshold: float, opts: _Options) -> _Clusters:
        """The cut per recording on the host (with bounds: the level search of cluster.agglomerative_cluster rule 7 in its place, host
        integers on the same Z), the cut's centroids, the grouped fold and the final centroids.  linkage: _pack_link's result; threshold:
        opts.threshold for run_many, one of its own for sweep."""
        eng, E_dev, rows, n_train, R = self.eng, p.E_dev, p.rows, p.n_train, len(p.rows)
        (link, off, Z), cuts, forced = linkage, {}, {}
        for g, r in enumerate(link):
            Zr = Z[int(off[g]) - g:int(off[g + 1]) - g - 1]
            cuts[r] = fcluster_distance(Zr, threshold)
            if opts.bounds is not None:                                             # K0 = the clusters the fold will keep: the large ones of the cut, or one
                eff_r = effective_min_size(opts.min_cluster_size, n_train[r])
                found = max(1, int((np.bincount(cuts[r]) >= eff_r).sum()))
                target = speaker_target(found, opts.bounds, n_train[r])
                if target is not None:
                    level, _ = level_search(Zr, eff_r, cut_level(Zr, threshold), target)
                    cuts[r] = _flat_partition(Zr, n_train[r], level)
                    forced[r] = {"found": found, "target": target, "method": "level", "level": level, "n_iter": None}
        cut_all, sizes, cl_off, eff, cent_off = [], [], [0], [], [0]
        for r in range(R):
            n = len(rows[r])
            cut = cuts[r] if r in cuts else np.zeros(n, np.int32)                  # one training row, or the candidates: one cluster
            sz = np.bincount(cut) if n else np.zeros(0, np.int64)
            m = min(int(opts.min_cluster_size), max(1, round(0.1 * n))) if r in cuts else 1     # cluster.fold_small_clusters, rule 1
            cut_all.append(cut.astype(np.int64) + cl_off[-1])
            sizes.append(sz)
            eff.append(m)
            cl_off.append(cl_off[-1] + len(sz))
            cent_off.append(cent_off[-1] + (max(1, int((sz >= m).sum())) if len(sz) else 0))
        cent_off = np.asarray(cent_off, np.int64)
        if not cl_off[-1]:
            return _Clusters(None, None, cent_off, {}, forced)
        rows_d = self._up(np.concatenate(rows).astype(np.int32))
        cut_d = self._up(np.concatenate(cut_all).astype(np.int32))
        _, cut64 = diarize_centroids(eng, E_dev, rows_d, cut_d, cl_off[-1], check_rows=False)
        _, final_d = diarize_fold_grouped(eng, cut64, np.concatenate(sizes), cl_off, eff, cent_off, cut_d, upload=self._up)
        return _Clusters(*diarize_centroids(eng, E_dev, rows_d, final_d, int(cent_off[-1]), check_rows=False), cent_off, {}, forced)

    def _pack_assign(self, p: _PackState, cl: _Clusters, opts: _Options):
        """Grouped assignment, stitching, renumbering by appearance and second stitching -> (labels, scores, cent, count, speakers) on the host."""
        dev = self._pack_assign_dev(p, cl, opts)
        if opts.smooth is None:
            return tuple(self._down(t) for t in dev)
        from .smooth import smooth_turns
        spk_dev, tal_dev = smooth_turns(self.eng, dev[4], p.tab, opts.smooth[2], opts.smooth[3], max(_speaker_cap(opts.max_speakers), 1))
        host = tuple(self._down(t) for t in dev[:4])
        flat = self._down(_native()[0].cat([spk_dev.reshape(-1), tal_dev.reshape(-1)]))    # the tallies ride with the speakers table: no further wait
        return host + (flat[:2 * p.tab.G].reshape(-1, 2), flat[2 * p.tab.G:].reshape(-1, 2))

    def _pack_assign_dev(self, p: _PackState, cl: _Clusters, opts: _Options):
        """_pack_assign without its downloads: (labels, scores, cent, count, speakers) on the device."""
        torch, eng, tab, c32, c64 = _native()[0], self.eng, p.tab, cl.c32, cl.c64
        if c64 is None:                                          # no cluster anywhere: the kernels still get a row to point at
            d = self.resnet.cfg.embed_dim
            c32, c64 = torch.zeros((1, d), dtype=torch.float32, device=eng.device), torch.zeros((1, d), dtype=torch.float64, device=eng.device)
        lab_dev, score_dev = diarize_assign_grouped(eng, p.E_dev, p.info_dev, c64, tab, opts.constrained)
        _, spk_dev, _ = diarize_reconstruct_grouped(eng, p.cls, lab_dev, tab, opts.max_speakers)
        first = diarize_first_seen(eng, spk_dev, tab)
        _, c32, c64 = diarize_renumber(eng, first, lab_dev, c32, c64, tab)         # ties in the top-2 go to the lower number: stitch again
        cnt_dev, spk_dev, _ = diarize_reconstruct_grouped(eng, p.cls, lab_dev, tab, opts.max_speakers)
        return lab_dev, score_dev, c32, cnt_dev, spk_dev

    def _pack_results(self, p: _PackState, cl: _Clusters, host, smooth: Optional[tuple] = None):
        """The pack's host arrays (host: _pack_assign's result; with smoothing the tallies [R, 2] stand behind them) cut into one
        DiarizationResult per recording."""
        pack, cent_off, info, cls, vres, forced = p.pack, cl.cent_off, p.info, p.cls, cl.vres, cl.forced
        labels, scores, cent, count, speakers = host[:5]
        out = []
        for r, x in enumerate(p.xs):
            if x.size == 0:
                out.append(self._smoothed(self._empty(), smooth))
                continue
            a, b, g0, g1, k0, k1 = (int(v) for v in (pack.chunk_off[r], pack.chunk_off[r + 1], pack.frame_off[r], pack.frame_off[r + 1], cent_off[r], cent_off[r + 1]))
            res = DiarizationResult(turns_from_frames(speakers[g0:g1], k1 - k0), k1 - k0, cent[k0:k1].copy(), labels[a:b].copy(), count[g0:g1].copy(),
                                    speakers[g0:g1].copy(), pack.starts_local[a:b].astype(np.int64), info[a:b].copy(), cls[a:b], scores[a:b].copy())
            if r in vres:
                res.pi, res.elbo = vres[r].pi, vres[r].elbo
            if r in forced:
                res.forced = forced[r]
            if cl.nres and r in cl.nres:
                res.nmesc = _nmesc_fields(cl.nres[r])
            out.append(self._smoothed(res, smooth, host[5][r] if smooth is not None else (0, 0)))
        return out
