"""`Backend` - the MI355X-native implementation of the toolkit's EmbeddingBackend contract
(speaker_detection_backends/base.py:22-200; registered through backends.yaml, loaded by
get_backend -> module.Backend(), base.py:272-293).

Audio windows (2 s, 16 kHz mono s16le) -> fbank -> ECAPA-TDNN -> L2-normalise -> cosine
affinity vs the enrolled profiles, all inside libsdk_hip.so.  No CPU fallback: without the built
library or without a gfx950 device the first compute call raises (the CLIs print
"Error during identification: ..." and exit 1, speaker_detection:1072-1074).

Environment:
  SDK_DEVICE          GPU index (default: $LOCAL_RANK, else 0)
  SDK_MODEL           "ecapa" (default: ECAPA-TDNN C = 1024) / "xvector" (plain TDNN x-vector, xvector.py): the second model family north_star names.
                      Same front end, same 192-d back end (k3 / k4 / store); model_version names the family, so vectors enrolled with one are
                      refused by the other (store.load_profile_batch).  SDK_XVECTOR_WEIGHTS: .npz in the xvector.py naming (default: seeded synthetic)
                      / "resnet34" (the WeSpeaker ResNet34 that PyAnnote 3.1 embeds with, resnet.py; 192-d).  SDK_RESNET_WEIGHTS: .npz in the public
                      state-dict naming of resnet.py (default: seeded synthetic).  Serves SDK_PRECISION 0 and 2, no bias correction, torch engine
                      only (SDK_NO_TORCH=1 is refused)
  SDK_DIARIZE_MODEL   the embedding network of diarize / diarize_many / open_streams: "resnet34" (default: the ResNet34 of $SDK_RESNET_WEIGHTS, whatever
                      SDK_MODEL is) / "ecapa" (the backend's own ECAPA-TDNN with masked attentive statistics pooling, ecapa_diar.py: needs
                      SDK_MODEL=ecapa and SDK_PRECISION 0 or 2; a diarization's centroids then live in the enrolled profiles' space, so
                      link_speakers(candidates=...) can name its speakers)
  SDK_ECAPA_WEIGHTS   .npz checkpoint in the weights.py naming (default: seeded synthetic weights -
                      there is no network here to fetch a pretrained model; a warning is printed)
  SDK_ECAPA_LAYOUT    "public": SDK_ECAPA_WEIGHTS is a checkpoint in the public ECAPA-TDNN state-dict naming (.ckpt / .pt via
                      torch.load(weights_only=True), .safetensors, .npz); SDK_ECAPA_PREFIX strips a key prefix
  SDK_WINDOW_S / SDK_HOP_S   analysis window / hop in seconds (default 2.0 / 1.0)
  SDK_NO_TORCH        1: the torch-free host path (lite.py) for enroll / identify / verify: same library calls, numpy on the host, device memory
                      from sdk_device_malloc - a warm-cache CLI process reaches its first row without the 0.8-s `import torch`.  The packed
                      weights come from the on-disk cache; a missing entry is built once in a child process (through the torch engine).
                      Serves SDK_PRECISION 0 and 2 (the precise mode needs the torch engine)
  SDK_BIAS_CORRECTION 1 (default) / 0: fold the constant part of the bf16 weight-rounding error into the layer biases (one calibration pass at the
                      first load of a weight set, cached): scores within ~8e-4 of the fp32 model instead of ~4e-3, no run-time cost
  SDK_CALIBRATION_WAV a 16 kHz mono s16 WAVE file whose two-second windows replace the built-in synthetic calibration audio of the bias correction
                      (with a trained checkpoint, calibrate on speech); the corrected blob is cached per calibration file
  SDK_PROFILE_PACK    1 (default) / 0: serve a candidate set from its packed profile matrix (embeddings/packs/, built at the first identify over
                      the set: one file mapped, no per-embedding I/O); SDK_PROFILE_PACK_MIN (16): smallest set that is packed
  SDK_PRECISION       0 (default: bf16 operands) / 1 (precise mode: fp16 hi+lo planes, within 1e-5,
                      ~3.6x the step time) / 2 (one fp16 plane: the default mode's kernels with fp16 storage and operands, within ~1e-4 with the
                      bias correction, ~1.04x the step time; both families).  All modes embed into the SAME space (they differ from each other at
                      the 4e-3 level), so model_version does not depend on it
  SDK_COHORT          a .npy [M, d] fp32 impostor cohort (Backend.make_cohort writes one): identify_speaker, identify_many, verify_speaker and
                      score_ranges then decide on the adaptively normalised score z (AS-norm, snorm.py) instead of the raw cosine.  Needs the
                      torch engine (SDK_NO_TORCH=1 is refused) and SDK_COHORT_THRESHOLD
  SDK_COHORT_TOPK     cohort scores per side that the statistics are taken over (default 300; min(K, M) is used)
  SDK_COHORT_THRESHOLD  the vote threshold on the z scale (a float).  No default: it depends on the model family and the cohort, and no trained
                      weights are on hand to tune one - a cohort without a threshold is refused.  tune_cohort_threshold(backend, ...) of
                      this module finds it on a labelled development set (trials_snorm.py); it needs no SDK_COHORT (cohort=)
  SDK_SCORE_PLDA_TRANSFORM / SDK_SCORE_PLDA   the two .npz files of a PLDA model of THIS family's embedding space (plda.save_plda writes them;
                      Backend.train_plda under the matching SDK_DIARIZE_MODEL makes one): both or neither.  identify_speaker, identify_many
                      and verify_speaker then decide on the PLDA log-likelihood ratio of a window against an enrolled SPEAKER - the speaker's
                      enrolled embeddings pooled, their number in the score (plda_score.py) - instead of the best single cosine.  They are
                      distinct from SDK_PLDA_TRANSFORM / SDK_PLDA, the model of the diarizer's embedding space, which may be another family.
                      Needs the torch engine (SDK_NO_TORCH=1 is refused); refused together with SDK_COHORT.  score_ranges stays on the cosine
  SDK_SCORE_PLDA_DIM  the PLDA dimensions kept, 64 or 128 (default 128)
  SDK_SCORE_PLDA_THRESHOLD  the vote threshold on the log-likelihood-ratio scale (a float, default 0: the point of equal likelihood under the
                      model).  The scale is UNCALIBRATED: 0 is not a tuned operating point.  Backend.tune_verification returns the thresholds
                      at the equal error rate and at the minimum detection cost of a labelled development set (trials.py);
                      calibrate_verification fits the map from this scale to a log-likelihood ratio (SDK_SCORE_CALIBRATION)
  SDK_SCORE_PLDA_COUNT  1 (default): a speaker's effective count n_s is the number of their enrolled embeddings ("by the book") / 0: n_s = 1
  SDK_SCORE_CALIBRATION  a calibration file (calibrate_verification(backend, ..., out_path=) of this module writes one; trials.py states the fit): rows of
                      identify_speaker / identify_many, and verify_speaker's answer, gain calibrated_llr = a * score + b (the score: the row's mean
                      cosine, or its mean llr under SDK_SCORE_PLDA*) and posterior = sigmoid(calibrated_llr + logit(SDK_SCORE_PRIOR)).  No decision,
                      threshold, order or existing key changes.  Refused when the file was fitted to the other rule, and together with SDK_COHORT
  SDK_SCORE_PRIOR     the prior of a target behind `posterior`, inside (0, 1) (default 0.5)
"""
from __future__ import annotations

import os
import sys
from contextlib import contextmanager
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from . import BACKEND_NAME, settings
from .families import FAMILIES
from .plugin_api import EmbeddingBackend
from .rules import Cosine, aggregate_matches, aggregate_matches_snorm, cached, rule_from_env  # noqa: F401  (the aggregations: imported from here)
from .store import load_profile_batch, publish_pack, save_vector, vector_path
from .wav import cut_ranges, cut_windows, decode_to_profile, range_starts, window_starts
from .weights import weights_digest

# Functions that take a Backend and are not methods of it (its public surface is pinned name for name, tests/test_rules_cpu.py): each lives
# with its subject and is importable from here, where callers and messages name it.
from .fuse import _per_recording, compare_diarizations, diarize_fused, fuse_diarizations  # noqa: F401
from .multiscale import cluster_ranges_multiscale  # noqa: F401
from .plda import plda_classes
from .samples import speaker_samples, write_samples  # noqa: F401
from .score import score_diarization_uem  # noqa: F401
from .smooth import smooth_diarization  # noqa: F401
from .trials import calibrate_verification  # noqa: F401
from .trials_snorm import _snorm_trials, score_verification_snorm, tune_cohort_threshold  # noqa: F401
from .words import attribute_transcript, attribute_transcripts, diarize_transcript, score_words  # noqa: F401


def _of_rule(name: str) -> property:
    """A Backend attribute that is a setting of its decision rule (rules.py): read and written there."""
    return property(lambda self: getattr(self.rule, name), lambda self, value: setattr(self.rule, name, value))


class Backend(EmbeddingBackend):
    cohort_path, cohort_threshold, cohort_topk = _of_rule("cohort_path"), _of_rule("cohort_threshold"), _of_rule("cohort_topk")
    score_plda_paths, score_plda_dim = _of_rule("score_plda_paths"), _of_rule("score_plda_dim")
    score_plda_threshold, score_plda_count = _of_rule("score_plda_threshold"), _of_rule("score_plda_count")
    _score_plda = _of_rule("loaded")                    # (plda.Plda, content digest) once score_plda() has read the files

    def __init__(self) -> None:
        self.model = os.environ.get("SDK_MODEL", "ecapa").strip().lower()
        if self.model not in FAMILIES:
            raise ValueError(f"SDK_MODEL={self.model!r}: expected 'ecapa', 'xvector' or 'resnet34'")
        self._family = FAMILIES[self.model]             # the selected family's row (families.py)
        self.diarize_model = os.environ.get("SDK_DIARIZE_MODEL", "resnet34").strip().lower()
        if self.diarize_model not in ("resnet34", "ecapa"):
            raise ValueError(f"SDK_DIARIZE_MODEL={self.diarize_model!r}: expected 'resnet34' (default) or 'ecapa'")
        if self.diarize_model == "ecapa":
            if self.model != "ecapa":
                raise ValueError(f"SDK_DIARIZE_MODEL=ecapa diarizes in the space of the backend's own ECAPA-TDNN: it requires SDK_MODEL=ecapa, got SDK_MODEL={self.model!r}")
            text = settings.precision_text()
            if ("0" if text is None else text).strip() not in ("0", "2"):
                raise ValueError(f"SDK_DIARIZE_MODEL=ecapa requires SDK_PRECISION 0 (bf16) or 2 (fp16): the masked pooling is not built for the precise mode, got "
                                 f"SDK_PRECISION={text!r}")
        if not settings.weights_path(self._family.weights_env):
            print(f"mi355x backend: {self._family.weights_env} not set - using seeded synthetic {self._family.label} weights "
                  "(scores are self-consistent but not trained)", file=sys.stderr)
        self._cache_hit = False
        self._engine = None
        self._extractor = None                          # the x-vector / ResNet34 extractor (None: the engine's own ECAPA-TDNN)
        self._weights = None
        self._digest: Optional[str] = None
        self.window_s = float(os.environ.get("SDK_WINDOW_S", "2.0"))
        self.hop_s = float(os.environ.get("SDK_HOP_S", "1.0"))
        self.rule = rule_from_env(os.environ)           # cosine, AS-norm or PLDA (rules.py); refuses a setting that does not hold together

    # ---- metadata (base.py:25-105) -------------------------------------------------------
    @property
    def name(self) -> str:
        return BACKEND_NAME

    @property
    def requires_api_key(self) -> bool:
        return False

    @property
    def embedding_dim(self) -> Optional[int]:
        return self._family.embed_dim

    @property
    def model_version(self) -> str:
        return f"{self.name}-{self._family.version_tag}-{self._weights_digest()}"

    @property
    def audio_profile(self):
        return BACKEND_NAME

    # ---- lazily built state --------------------------------------------------------------
    def _host_weights(self):
        if self._weights is None:
            self._weights = self._family.host_weights()              # the checkpoint its variable names, shape-checked, else seeded synthetic
        return self._weights

    def _cache_key(self) -> str:
        """Identity of the weights for the packed-blob cache, without reading them (weights_cache.py); None: the family's blob is not cached."""
        from . import weights_cache
        if not self._family.cached:
            return None
        path = settings.weights_path(self._family.weights_env)
        return weights_cache.key_for_file(path) if path else weights_cache.key_for_seed(0, self._family.config)

    def _weights_digest(self) -> str:
        """Content hash of the weights (part of model_version).  A process that finds the packed blob in the cache takes the digest
        from the cache entry too: no 20.8 M-parameter generate / parse, no SHA-256 over 83 MB, no re-pack (cold start: tools/cold_start.py)."""
        if self._digest is None:
            from . import weights_cache
            key = self._cache_key()
            meta = weights_cache.load_meta(key) if key else None
            if meta and meta.get("digest") and self._weights is None:
                self._digest = meta["digest"]
                self._cache_hit = True
            else:
                self._digest = weights_digest(self._host_weights())
        return self._digest

    def numerics(self) -> Dict[str, Any]:
        """The numerical setting embeddings are made under (stored beside every enrolled vector; identify warns when a candidate was made
        under another one): model_version names the WEIGHTS - both settings embed into the same space, ~4e-3 apart."""
        prec = settings.precision()
        return {"precision": prec, "bias_correction": settings.bias_correction() and prec in (0, 2) and self._family.bias_correction}

    @property
    def lite(self) -> bool:
        return settings.lite()

    def _lite_engine(self):
        """lite.LiteEngine on the cached packed weights; a cache miss is filled ONCE by a child process that runs the torch engine (pack, bias-correction
        calibration pass, store) - this process must not import torch itself (one HIP runtime per process)."""
        fam = self._family
        if not fam.lite:
            raise ValueError(f"SDK_NO_TORCH=1 with SDK_MODEL={fam.name}: the torch-free host path does not serve the {fam.label} family; unset SDK_NO_TORCH")
        from .lite import LiteEngine
        dev, prec = settings.device(), settings.precision()
        if prec not in (0, 2):
            raise ValueError(f"SDK_NO_TORCH=1 serves the single-plane contracts (SDK_PRECISION=0 or 2); SDK_PRECISION={prec} needs the torch engine")
        if fam.lite_load is not None:                 # a family whose blob is packed here, not cached
            eng = LiteEngine(dev, precision=prec)
            fam.lite_load(eng, self._host_weights())
            return eng
        eng = LiteEngine(dev, cache_key=self._cache_key(), precision=prec)
        if not eng.has_cached_weights():
            import subprocess
            root = str(Path(__file__).resolve().parent.parent)
            env = {k: v for k, v in os.environ.items() if k != "SDK_NO_TORCH"}
            env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
            code = f"import importlib; b = importlib.import_module('{__package__}.backend').Backend(); b.engine().desc"
            try:                                  # bounded: a stuck child must not hang the CLI; the build takes ~2 s
                r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                                   timeout=settings.cache_build_timeout_s())
                err = r.stderr.strip()[-400:] if r.returncode != 0 else ""
            except subprocess.TimeoutExpired:
                r, err = None, "the child process did not finish in time (SDK_CACHE_BUILD_TIMEOUT_S)"
            if r is None or r.returncode != 0 or not eng.has_cached_weights():
                raise RuntimeError("SDK_NO_TORCH=1: building the packed-weight cache entry in a child process failed "
                                   f"(is the cache writable? SDK_CACHE_DIR / SDK_WEIGHTS_CACHE): {err}")
        eng.load_weights()
        self._cache_hit = eng.cache_hit
        return eng

    def engine(self):
        if self._engine is None and self.lite:
            self._engine = self._lite_engine()
        if self._engine is None:
            from .ops import Engine   # imports torch + dlopens libsdk_hip.so; raises SdkError if absent
            fam, dev, prec = self._family, settings.device(), settings.precision()
            if prec == 1 and 1 not in fam.precisions:
                raise ValueError(f"SDK_PRECISION=1 (the precise mode) is not built for SDK_MODEL={fam.name}: use SDK_PRECISION=0 or 2")
            if fam.extractor_name is None:               # the engine's own ECAPA-TDNN: packed on first use, from the cache where it can
                self._engine = Engine(dev, cache_key=self._cache_key(), weights_fn=self._host_weights, digest_fn=self._weights_digest)
            else:
                self._engine = Engine(dev)               # front end, k3, k4; its ECAPA weights are never packed (lazy)
            if prec:
                self._engine.set_precision(prec)
            if fam.extractor_name is not None:
                self._extractor = fam.extractor(self._engine, self._host_weights(), prec)    # bias correction: $SDK_BIAS_CORRECTION (default on)
        return self._engine

    def _embed_pcm(self, pcm_dev):
        """[B, S] int16 device tensor -> (E fp32, Eb bf16, resid): the selected model family's fbank -> forward -> L2 sequence."""
        eng = self.engine()
        return self._extractor.embed_pcm(pcm_dev) if self._extractor is not None else eng.embed_pcm(pcm_dev)

    # ---- the GPU path ----------------------------------------------------------------------
    def embed_windows(self, pcm: np.ndarray):
        """pcm [B, S] int16 (host) -> torch device tensors (E fp32, Eb bf16, resid).
        Recordings of any length: the forward's scratch is ~6.7 MB per 2-s window, so the windows go through in batches
        of SDK_MAX_BATCH (default 2048 = 13.7 GB of scratch; a 1-h file at a 1-s hop is two batches)."""
        eng = self.engine()
        step = settings.max_batch()
        if self.lite:
            raise RuntimeError("embed_windows returns device tensors: not available with SDK_NO_TORCH=1 (use embed_windows_host)")
        import torch
        if pcm.shape[0] <= step:
            return self._embed_pcm(torch.from_numpy(np.ascontiguousarray(pcm)).to(eng.device))
        parts = [self._embed_pcm(torch.from_numpy(np.ascontiguousarray(pcm[a:a + step])).to(eng.device))
                 for a in range(0, pcm.shape[0], step)]
        return tuple(torch.cat([p[i] for p in parts], dim=0) for i in range(3))

    def embed_windows_host(self, pcm: np.ndarray, profiles=None, k: int = 1):
        """pcm [B, S] int16 -> unit-norm embeddings [B, d] fp32 on the HOST and, when `profiles` (a store.ProfileBatch, or a [P, d] matrix) is
        given, the cosine top-k of every window (idx [B, k] int32, score [B, k] fp32) - the torch-free form of embed_windows + score_windows
        (SDK_NO_TORCH=1), same bounded batches.  A ProfileBatch served from its pack is uploaded as packed (no normalisation pass); one loaded
        file by file is normalised on the device once and its pack is published."""
        eng = self.engine()
        step = settings.max_batch()
        Es, idxs, scs = [], [], []
        batch = profiles if hasattr(profiles, "matrix") else None
        for a in range(0, pcm.shape[0], step):
            Es.append(eng.embed_pcm(pcm[a:a + step]))
            if batch is not None:
                i, s_ = eng.score_last(batch.matrix, k, norm=batch.norm, tag=batch.uid,
                                       on_norm=(lambda E, Eb, r: publish_pack(batch, E, Eb, r)) if batch.pack_ref else None)
                idxs.append(i); scs.append(s_)
            elif profiles is not None:
                i, s_ = eng.score_last(profiles, k)
                idxs.append(i); scs.append(s_)
        E = np.concatenate(Es) if Es else np.zeros((0, self.embedding_dim), np.float32)
        return (E, np.concatenate(idxs), np.concatenate(scs)) if profiles is not None else (E, None, None)

    def _windows(self, audio_path: Path, segments):
        """Decoded recording + the table of its analysis windows (first samples; nothing is cut on the host)."""
        samples = decode_to_profile(Path(audio_path), self.engine(), self.get_audio_profile())   # other rates / layouts: GPU resampler
        starts, spans, W = window_starts(len(samples), segments, window_s=self.window_s, hop_s=self.hop_s)
        if len(spans) == 0:
            raise ValueError(f"{audio_path}: no analysable audio (every segment shorter than 0.5 s)")
        return samples, starts, W, spans

    def embed_tables(self, samples: np.ndarray, tables: Dict[int, np.ndarray]):
        """The ingest path: one recording in host memory + window-start tables {window samples S: int32 [B_S]} ->
        {S: (E, Eb, resid)} device tensors.  The recording crosses PCIe once, through pinned staging on a copy stream (the next call's upload
        overlaps this call's forward); the overlapping windows are cut on the device (sdk_fbank_windows) in batches of SDK_MAX_BATCH."""
        eng = self.engine()
        if self.lite:
            raise RuntimeError("embed_tables returns device tensors: not available with SDK_NO_TORCH=1 (use embed_tables_host)")
        step = settings.max_batch()
        return eng.embed_from_host(samples, tables, step, forward=self._extractor.forward if self._extractor is not None else None)

    def embed_tables_host(self, samples: np.ndarray, tables: Dict[int, np.ndarray], batch=None, k: int = 1):
        """The same for the torch-free host path: {S: (E host, idx, score)}; with a ProfileBatch every batch of windows is scored while resident."""
        eng = self.engine()
        step = settings.max_batch()
        kw = None
        if batch is not None:
            kw = {"norm": batch.norm, "tag": batch.uid, "on_norm": (lambda E, Eb, r: publish_pack(batch, E, Eb, r)) if batch.pack_ref else None}
        return eng.embed_from_host(samples, tables, step, profiles=batch.matrix if batch is not None else None, k=k, score_kw=kw)

    def embed_ranges(self, samples: np.ndarray, ranges: List[Tuple[float, float]]):
        """Single-speaker ranges (sentences, enrollment segments) -> embeddings of true-length windows.
        The windows are bucketed by length (wav.cut_ranges: 0.5 / 1 / 1.5 / 2 s = 51 / 101 / 151 / 201 frames) and each
        bucket is ONE forward launch sequence; no window contains audio from outside its range.
        Returns (E, Eb, resid) device tensors in window order, windows [(range index, start s, end s)], dropped ranges."""
        import torch
        starts_by, wins, dropped = range_starts(len(samples), ranges, hop_s=self.hop_s)
        if not wins:
            return None, None, None, [], dropped
        parts = self.embed_tables(samples, starts_by)                      # the recording is uploaded once; one launch sequence per bucket
        order = {S: [] for S in parts}
        for w, (_, S, row, _, _) in enumerate(wins):
            order[S].append((row, w))
        dev = next(iter(parts.values()))[0].device
        out = []
        for i in range(3):
            ref = next(iter(parts.values()))[i]
            full = torch.empty((len(wins),) + tuple(ref.shape[1:]), dtype=ref.dtype, device=dev)
            for S, pairs in order.items():
                rows = torch.tensor([r for r, _ in pairs], device=dev)
                dst = torch.tensor([w for _, w in pairs], device=dev)
                full[dst] = parts[S][i][rows]
            out.append(full)
        return out[0], out[1], out[2], [(ri, a, b) for ri, _, _, a, b in wins], dropped

    def score_ranges(self, samples: np.ndarray, ranges: List[Tuple[float, float]], batch, k: int = 1):
        """Single-speaker ranges -> per window (best profile rows [W, k], scores [W, k]) on the host + windows [(range index, start s, end s)]:
        embed_ranges + score_windows in one call, on either host path (torch engine or SDK_NO_TORCH=1).  With a cohort configured (SDK_COHORT)
        the rows are the normalised top-k and the scores are z values (score_windows_snorm), not cosines.  With a scoring PLDA configured
        (SDK_SCORE_PLDA*) they are COSINES against the enrolled embeddings, not log-likelihood ratios; with SDK_NO_TORCH=1 the host path
        below answers, with cosines.  So this is the one call that does not follow the Backend's rule ("known gaps": the PLDA
        rule is not applied here, and identify.make_rows_fn(per_label=True) votes on what comes back at the raw cosine threshold, z or not)."""
        if not self.lite:
            E, Eb, re, wins, _ = self.embed_ranges(samples, ranges)
            if not wins:
                return np.zeros((0, k), np.int32), np.zeros((0, k), np.float32), []
            if self.cohort_path:
                idx, z, _ = self.score_windows_snorm(E, batch, k)
                return idx, z, wins
            idx, sc = self.score_windows(E, Eb, re, batch, k)
            return idx, sc, wins
        starts_by, wins, _ = range_starts(len(samples), ranges, hop_s=self.hop_s)
        if not wins:
            return np.zeros((0, k), np.int32), np.zeros((0, k), np.float32), []
        parts = self.embed_tables_host(samples, starts_by, batch, k)                                   # one bucket = one forward + one top-k
        idx = np.stack([parts[S][1][row] for _, S, row, _, _ in wins])
        sc = np.stack([parts[S][2][row] for _, S, row, _, _ in wins])
        return idx, sc, [(ri, a, b) for ri, _, _, a, b in wins]

    def _ranges_plda(self, plda, d: int):
        """The plda.Plda of cluster_ranges(clustering="vbx") for embeddings of width d: the one given, else Backend.diarizer()'s."""
        if plda is None:
            plda = self.diarizer().plda_model()
        if plda.d_in != d:
            raise ValueError(f"cluster_ranges: the PLDA model takes d_in={plda.d_in}, the embeddings have d={d}: pass plda= for this embedding family")
        return plda

    def cluster_ranges(self, samples: np.ndarray, ranges: List[Tuple[float, float]], threshold: float = 0.7045654963945799,
                       min_cluster_size: int = 12, speakers=None, clustering: str = "ahc", loop_prob: float = 0.99, plda=None):      # cluster.VBX_LOOP_PROB
        """Speaker labels for a transcript's segments with no enrolled profiles: embed_ranges -> cluster.agglomerative_cluster (centroid
        linkage on the GPU, flat cut at `threshold`, clusters under min_cluster_size folded into the nearest large one).
        Returns (labels [W] int32 per window, windows [(range index, start s, end s)], range_labels [len(ranges)] int32): a range takes the
        majority label of its windows (ties -> the smaller label), -1 when it has no window.
        The default threshold and size are PyAnnote 3.1's, tuned for ITS trained ResNet34 embedding (SDK_MODEL=resnet34 with the trained
        weights); with another family or the synthetic weights pass a threshold of your own.
        clustering="vbx" (default "ahc", the path above): the windows, which embed_ranges returns in time order, are the sequence of a VBx
        clustering with its HMM (cluster.vbx_cluster with loop_prob, default cluster.VBX_LOOP_PROB = 0.99: BUT's value for a 0.25-s step,
        unpinned here).  `threshold` then cuts the linkage that only initialises it (pass cluster.VBX_AHC_THRESHOLD, 0.6); min_cluster_size is
        not used; labels are the arg-max of gamma over the kept speakers.  plda: a plda.Plda for this family's embedding width; None takes
        Backend.diarizer()'s ($SDK_PLDA_TRANSFORM and $SDK_PLDA, else the seeded synthetic model for the ResNet34's width).  One window:
        label 0.  The same triple comes back.
        speakers: the number of speakers, None, an int k (exactly k) or a pair (lo, hi), either side None (cluster.parse_speakers and the
        bounds stated above it; pyannote's max_speakers is speakers=(None, hi)).  When the count found lies outside, "ahc" takes the level
        search of cluster.agglomerative_cluster rule 7 and "vbx" the k-means of cluster.kmeans_cluster on the window rows, whose labels come
        back; fewer than two windows: nothing is forced.
        clustering="nmesc": the eigengap spectral clustering of cluster.nmesc_cluster on the window rows, with no threshold: `threshold`,
        min_cluster_size, loop_prob and plda are not used, and `speakers` bounds the eigengap search itself.  Its multi-scale form - every
        range at several window lengths, the affinities fused on the shortest one's windows - is backend.cluster_ranges_multiscale(be, ...)."""
        if self.lite:
            raise ValueError("cluster_ranges needs the torch engine: not available with SDK_NO_TORCH=1")
        if clustering not in ("ahc", "vbx", "nmesc"):
            raise ValueError(f"cluster_ranges: clustering={clustering!r} (\"ahc\", \"vbx\" or \"nmesc\")")
        from .cluster import agglomerative_cluster, nmesc_cluster, parse_speakers, vbx_cluster
        speakers = parse_speakers(speakers, "cluster_ranges")
        E, _, _, wins, _ = self.embed_ranges(samples, ranges)
        range_labels = np.full(len(ranges), -1, dtype=np.int32)
        if not wins:
            return np.zeros(0, np.int32), [], range_labels
        if clustering == "ahc":
            labels = agglomerative_cluster(self.engine(), E, threshold, min_cluster_size, speakers=speakers).labels
        elif len(wins) == 1:
            labels = np.zeros(1, np.int32)
        elif clustering == "nmesc":
            labels = nmesc_cluster(self.engine(), E.contiguous(), speakers=speakers).labels
        else:
            labels = vbx_cluster(self.engine(), E.contiguous(), self._ranges_plda(plda, int(E.shape[1])), threshold, loop_prob=loop_prob,
                                 speakers=speakers).labels
        per = {}
        for (ri, _, _), lab in zip(wins, labels):
            per.setdefault(ri, []).append(int(lab))
        for ri, labs in per.items():
            range_labels[ri] = int(np.argmax(np.bincount(labs)))        # first maximum = the smaller label
        return labels, wins, range_labels

    def segmentation(self):
        """The resident PyanNet segmentation model (segmentation.py), whatever SDK_MODEL is: weights from $SDK_SEGMENTATION_WEIGHTS (.npz in
        pyannote's naming), else seeded synthetic; precision from SDK_PRECISION (0 or 2; the precise mode is not built for it)."""
        if self.lite:
            raise ValueError("speech_ranges needs the torch engine: not available with SDK_NO_TORCH=1")
        if getattr(self, "_segmentation", None) is None:
            from .segmentation import Segmentation, load_weights, synthetic_weights as seg_synthetic
            prec = settings.precision()
            if prec == 1:
                raise ValueError("SDK_PRECISION=1 (the precise mode) is not built for the segmentation model: use SDK_PRECISION=0 or 2")
            path = settings.weights_path("SDK_SEGMENTATION_WEIGHTS")
            w = load_weights(path) if path else seg_synthetic(0)
            self._segmentation = Segmentation(self.engine(), w, precision=prec)
        return self._segmentation

    def speech_ranges(self, samples: np.ndarray, step_s: float = 1.0):
        """Speech and overlapped speech of a recording with no transcript: (speech [(start_s, end_s)], overlap [(start_s, end_s)]).
        The recording (16 kHz mono int16) is uploaded once; 10-s chunks starting at 0, step_s, 2 step_s, ... plus one ending at the recording's
        end (one zero-padded chunk below 10 s) are cut on the device and segmented in batches of $SDK_SEGMENTATION_BATCH (default 256).  Each
        chunk's per-frame speaker count (its powerset argmax) is aggregated on the global 270-sample frame grid by segmentation.aggregate_counts:
        a frame is speech when at least half of the chunks that see it count >= 1 speaker, overlap when at least half count >= 2.  The rule
        needs no alignment of local speakers between chunks (that belongs to the full diarization pipeline).  `speech` can be passed straight
        to cluster_ranges."""
        import torch
        from .segmentation import aggregate_counts, chunk_starts, speaker_count
        model = self.segmentation()
        x = np.ascontiguousarray(samples, dtype=np.int16).reshape(-1)
        if x.size == 0:
            return [], []
        st = chunk_starts(x.size, step_s)
        rec = torch.from_numpy(x).to(model.eng.device)
        step = settings.segmentation_batch()
        counts = []
        for a in range(0, len(st), step):
            s = torch.from_numpy(st[a:a + step].astype(np.int32)).to(model.eng.device)
            counts.append(speaker_count(model.forward(rec, s)).cpu().numpy())
        return aggregate_counts(np.concatenate(counts), st, x.size)

    def diarizer(self):
        """The resident diarization pipeline (diarize.py): Backend.segmentation() and the embedding network SDK_DIARIZE_MODEL names.
        "resnet34" (default): the ResNet34 built from $SDK_RESNET_WEIGHTS (.npz in the public naming, else seeded synthetic) whatever
        SDK_MODEL is; precision from SDK_PRECISION (0 or 2).  "ecapa" (needs SDK_MODEL=ecapa, SDK_PRECISION 0 or 2): ecapa_diar.EcapaEmbedder
        on the engine's own ECAPA-TDNN - its weights ($SDK_ECAPA_WEIGHTS), bias correction and embedding space, the one profiles are
        enrolled in - with S masked attentive statistics poolings per chunk (sdk_ecapa_forward_masked).  The PLDA model of
        clustering="vbx" comes from $SDK_PLDA_TRANSFORM (xvec_transform.npz: mean1, mean2, lda) and $SDK_PLDA (plda.npz: mu, tr, psi), both or
        neither, with $SDK_PLDA_DIM (64 or 128, default 128) dimensions kept; else a seeded synthetic model, made on first use."""
        if self.lite:
            raise ValueError("diarize needs the torch engine: not available with SDK_NO_TORCH=1")
        if getattr(self, "_diarizer", None) is None:
            from .diarize import Diarizer
            model = self.segmentation()
            resnet34 = FAMILIES["resnet34"]
            if self.diarize_model == "ecapa":
                from .ecapa_diar import EcapaEmbedder
                net = EcapaEmbedder(self.engine())                # the engine's own blob: the enrolled space, bias correction included
            elif self._family is resnet34:
                net = self._extractor                            # built by engine() from the same weights
            else:
                prec = settings.precision()
                net = resnet34.extractor(self.engine(), resnet34.host_weights(), prec)
            files = settings.diarizer_plda()                     # refuses one file without the other
            model_plda = None
            if files is not None:
                from .plda import load_plda
                model_plda = load_plda(*files)
            self._diarizer = Diarizer(self.engine(), model, net, model_plda)
        return self._diarizer

    def _recordings(self, samples_or_paths) -> list:
        """A list of recordings, each 16 kHz mono int16 samples or the path of an audio file: the paths decoded to the audio profile."""
        return [decode_to_profile(Path(x), self.engine(), self.get_audio_profile()) if isinstance(x, (str, Path)) else x for x in samples_or_paths]

    @staticmethod
    @contextmanager
    def _restored_precision(dz):
        """The diarizer steps in its network's numerical contract: on the way out its engine goes back to the precision it had."""
        prec = dz.eng.precision
        try:
            yield
        finally:
            if dz.eng.precision != prec:
                dz.eng.set_precision(prec)                       # the front end's format goes back to the selected family's contract

    def diarize(self, samples_or_path, **kw):
        """Who spoke when, with no transcript and no enrolled profiles: a recording (16 kHz mono int16 samples, or the path of an audio file,
        decoded to the audio profile) -> diarize.DiarizationResult (turns [(start_s, end_s, speaker)], n_speakers, unit centroids in the
        diarizer's embedding space - that of score_windows and the enrolled profiles under SDK_MODEL=resnet34, or SDK_MODEL=ecapa with
        SDK_DIARIZE_MODEL=ecapa - labels, count, speakers); diarize.to_rttm(result.turns, uri) writes RTTM.  Keywords: step_s,
        threshold, min_cluster_size, max_speakers, logp, constrained, clustering, vbx, speakers, nmesc (diarize.Diarizer.run; clustering="nmesc" is the eigengap spectral clustering, which needs no threshold).  The default threshold is PyAnnote 3.1's, tuned
        for its trained ResNet34 ($SDK_RESNET_WEIGHTS); with the synthetic weights pass a threshold of your own.  constrained=True
        (PyAnnote's constrained_argmax; default False): the local speakers of a chunk get pairwise different clusters, the one-to-one
        matching of largest total cosine, computed on the device; the result then carries scores [C, 3].  clustering="vbx" (default "ahc"):
        the cut of the linkage at `threshold` (pass cluster.VBX_AHC_THRESHOLD, 0.6) only initialises a VBx clustering in PLDA space
        (cluster.vbx_cluster; the model of Backend.diarizer), whose speakers' centroids the assignment then reads; vbx: a dict of Fa, Fb,
        max_iters, epsilon, init_smoothing.  The result then carries scores, pi and elbo.  speakers=k, or (lo, hi) with either side None:
        the number of speakers of the recording ("bounds" in diarize.py; pyannote's max_speakers is speakers=(None, hi), max_speakers here
        is the cap per frame); result.forced says whether the clustering was overruled.  min_duration_off, min_duration_on (seconds,
        default 0: nothing is done): a speaker's pauses no longer than the first are filled, then the turns shorter than the second are
        dropped, on the device before the speakers table comes down (smooth.py states the rule); result.smoothing says what was done, and
        smooth_diarization of this module does the same to finished results.  Parity with PyAnnote is unpinned."""
        dz = self.diarizer()
        rec, = self._recordings([samples_or_path])
        with self._restored_precision(dz):
            return dz.run(rec, **kw)

    def diarize_many(self, samples_or_paths, **kw):
        """diarize for a folder of recordings in one device pass per pack: a list of recordings (16 kHz mono int16 samples or paths of audio
        files, decoded to the audio profile) -> a list of diarize.DiarizationResult, in order.  Chunks of different recordings share the
        segmentation and embedding batches, one grouped linkage launch clusters all recordings, and assignment, fold and stitching run in
        grouped kernels; the host waits for the device a fixed number of times per pack, not per recording (diarize.Diarizer.run_many,
        which also states how the results relate to diarize's).  Keywords as diarize, min_duration_off and min_duration_on among them (the
        pack's table is smoothed in one launch sequence and no wait is added); logp is a list with one array per recording."""
        dz = self.diarizer()
        recs = self._recordings(samples_or_paths)
        with self._restored_precision(dz):
            return dz.run_many(recs, **kw)

    def _references(self, who: str, references, uris, n: int):
        """One turn list per recording from `references`: a list of turn lists [(start_s, end_s, name)], or an RTTM path / text / {uri: turns}
        with the recordings' uris."""
        from .score import references_for
        if isinstance(references, (str, Path, dict)):
            if uris is None or len(uris) != n:
                raise ValueError(f"{who}: an RTTM reference needs uris, one per recording ({n}), got {None if uris is None else len(uris)}")
            return references_for(references, list(uris))
        references = list(references)
        if len(references) != n:
            raise ValueError(f"{who}: {len(references)} references for {n} recordings")
        return references

    def score_diarization(self, results, references, uris=None, collar_s: float = 0.0, skip_overlap: bool = False):
        """How good diarize / diarize_many / a finished stream did: the diarization error rate of every result against its reference -> a list
        of score.DerResult (scored, total, missed, false_alarm, confusion, correct, der, mapping, co); score.pool(list) is the corpus
        figure.  references: one list of (start_s, end_s, name) per result, or the path or text of an RTTM file (or {uri: turns}) with
        `uris` naming the results' recordings in it.  collar_s: md-eval's collar, on each side of every reference boundary; skip_overlap:
        frames with two or more reference speakers are not scored.  Scored on the device in one pack (score.py states the rule; parity
        with md-eval and pyannote.metrics is unpinned).  With an evaluation map (UEM) or the Jaccard error rate: score_diarization_uem
        of this module."""
        results = list(results)
        return self.diarizer().score(results, self._references("score_diarization", references, uris, len(results)), collar_s, skip_overlap)

    def tune_diarization(self, samples_or_paths, references, thresholds, uris=None, **kw):
        """The DER of diarize_many at every threshold of `thresholds` against `references` (as score_diarization takes them) ->
        score.SweepResult (thresholds, per_recording [T][R], pooled [T], best): the tool for choosing the clustering threshold on a
        development set with weights of your own.  The recordings are embedded and linked once per pack; every threshold costs only the cut,
        the grouped assignment, the stitching and the scoring kernels (diarize.Diarizer.sweep).  Keywords: step_s, min_cluster_size,
        max_speakers, logp, constrained, collar_s, skip_overlap; clustering="ahc" without speakers= only.  uem, jer: as score_diarization's (a
        UEM file is read with `uris`); metric="der" or "jer": what `best` minimises, the pooled DER or the pooled Jaccard error rate.
        smoothing: None, or a list of (min_duration_off, min_duration_on) pairs: every threshold is then scored under every pair (the
        table smoothed on the device where it lies, no further wait) -> score.SmoothSweepResult (thresholds, smoothing, per_recording
        [T][S][R], pooled [T][S], best = (threshold, min_duration_off, min_duration_on)): whether half a second of gap filling helps more
        than another cut."""
        dz = self.diarizer()
        recs = self._recordings(samples_or_paths)
        refs = self._references("tune_diarization", references, uris, len(recs))
        with self._restored_precision(dz):
            return dz.sweep(recs, refs, thresholds, uris=uris, **kw)

    def score_verification(self, audio_paths, speaker_ids, candidates, score_range=None, p_target: float = 0.01, c_miss: float = 1.0,
                           c_fa: float = 1.0, max_refine: int = 8):
        """How well the decision rule of identify_speaker / verify_speaker separates the enrolled speakers on labelled recordings ->
        trials.VerificationResult (eer, eer_threshold, min_dcf, min_dcf_lower, min_dcf_exact, min_dcf_threshold, the DET arrays, the counts).
        audio_paths: recordings of ONE speaker each; speaker_ids: that speaker's id per recording as the candidates' profiles name it (an id
        no candidate has: the recording's windows are nontarget trials against everybody; None: they take part in no trial).
        Every window of every recording, embedded on identify's path, is one test row (its session: the index of its recording); the model
        rows are the candidates' enrolled embeddings (profile_tensors) under the cosine rule, their speakers (speaker_table) under the PLDA
        rule (SDK_SCORE_PLDA*) - the rule identify_speaker would use.  Scored on the device in trials.py's integer form (the rule is stated
        there; parity with outside toolkits is unpinned); score_range defaults to trials.COSINE_RANGE / trials.PLDA_RANGE.  With a cohort
        configured (SDK_COHORT): ValueError - AS-norm trials are not built."""
        from . import trials
        eng, tensors, kind = self._verification_trials("score_verification", audio_paths, speaker_ids, candidates)
        return trials.evaluate_scores(eng, *tensors, kind, score_range, p_target, c_miss, c_fa, max_refine)

    def _verification_trials(self, who: str, audio_paths, speaker_ids, candidates):
        """The trials of score_verification and calibrate_verification in matrix form -> (engine, (A, B, r, la, sa, lb, sb), kind)."""
        self.rule.refuse_trials()
        eng, E, speaker_ids, counts, batch = self._trial_windows(who, audio_paths, speaker_ids, candidates)
        A, B, r, lb, kind, index = self.rule.trial_matrices(self, E, batch)
        return eng, (A, B, r) + self._trial_labels(E.device, speaker_ids, counts, lb, index), kind

    def _trial_windows(self, who: str, audio_paths, speaker_ids, candidates):
        """The test side of verification trials, whatever the rule: every window of every recording embedded on identify's path ->
        (engine, E [windows, d], the speaker ids as a list, the windows per recording, the candidates' ProfileBatch)."""
        import torch
        if self.lite:
            raise ValueError(f"{who}: needs the torch engine; unset SDK_NO_TORCH")
        audio_paths, speaker_ids = list(audio_paths), list(speaker_ids)
        if len(audio_paths) != len(speaker_ids) or not audio_paths:
            raise ValueError(f"{who}: {len(audio_paths)} recordings with {len(speaker_ids)} speaker ids (one per recording, at least one)")
        batch = self._load_candidates(candidates)
        if len(batch) == 0:
            raise ValueError(f"{who}: no candidate embedding to score against")
        eng = self.engine()
        rows = []
        for path in audio_paths:
            samples, starts, W, _ = self._windows(Path(path), None)
            rows.append(self.embed_tables(samples, {W: starts})[W][0])
        return eng, torch.cat(rows, dim=0).contiguous(), speaker_ids, [int(r.shape[0]) for r in rows], batch

    @staticmethod
    def _trial_labels(device, speaker_ids, counts, lb, index):
        """(la, sa, lb, sb) int32 device tensors: a window's label is its recording's speaker in `index` ({speaker id: label}, as the rule's
        trial_matrices numbered the model rows `lb`), its session the index of its recording; the model rows have no session."""
        import torch
        la, sa = [], []
        for f, sid in enumerate(speaker_ids):                    # an id no candidate has: a label of its own, past the model rows'
            la += [-1 if sid is None else index.setdefault(sid, len(index))] * counts[f]
            sa += [f] * counts[f]
        i32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(device)        # noqa: E731
        sb = np.full(len(lb), -1)
        return i32(la), i32(sa), i32(lb), i32(sb)

    def tune_verification(self, audio_paths, speaker_ids, candidates, score_range=None, p_target: float = 0.01, c_miss: float = 1.0,
                          c_fa: float = 1.0, max_refine: int = 8) -> Dict[str, Any]:
        """The thresholds of the identify / verify decision on a labelled development set (the arguments of score_verification) ->
        {"kind", "eer", "eer_threshold", "min_dcf", "min_dcf_threshold", "min_dcf_lower", "min_dcf_exact", "n_target", "n_nontarget", "n_nan",
        "n_excluded", "n_test_rows", "n_model_rows", "score_range", "result": the VerificationResult}.  kind "cosine": the thresholds are
        directly usable as threshold= of identify_speaker and verify_speaker.  The evaluation scores the float64 product of the fp32 unit
        rows; identify's fp32 cosines of the same rows agree with it only to fp32 rounding (a few 1e-7), so a window within that of the
        threshold may vote differently.  kind "plda": they are usable as SDK_SCORE_PLDA_THRESHOLD - the tuned operating point that the
        uncalibrated default 0 is not."""
        from .trials import summary
        return summary(self.score_verification(audio_paths, speaker_ids, candidates, score_range, p_target, c_miss, c_fa, max_refine))

    def train_plda(self, samples_or_paths, references, uris=None, out_dir=None, D0: int = 128, lda_dim: int = 128, n_iters: int = 10,
                   step_s: float = 1.0, speaker_key=None, logp=None):
        """A PLDA model for clustering="vbx" fitted to THIS embedding space from recordings with reference annotations (the inputs of
        tune_diarization; references as score_diarization takes them) -> (plda.Plda, report).  The recordings are embedded in packs and every
        training row is labelled with the reference speaker that covers it (diarize.Diarizer.plda_rows); a class is (recording, reference
        name) - one person in two recordings is two classes - unless speaker_key(uri, name) maps several to one key (uri: the recording's
        entry of `uris`, else its index).  plda.fit then runs on the device (plda.py states the rule and what it refuses: at least D0 + 1
        classes and N - K' >= the embedding width).  report: rows_used, rows_dropped, classes, counts, objf, and with out_dir the two paths
        written, xvec_transform.npz and plda.npz, which $SDK_PLDA_TRANSFORM / $SDK_PLDA accept."""
        from . import plda as plda_mod
        dz = self.diarizer()
        recs = self._recordings(samples_or_paths)
        refs = self._references("train_plda", references, uris, len(recs))
        with self._restored_precision(dz):
            got = dz.plda_rows(recs, refs, step_s=step_s, logp=logp)
        labels, keys = plda_classes(got["recording"], got["speaker"], got["names"], uris, speaker_key)
        if not len(labels):
            raise ValueError("train_plda: no training row is covered by a reference speaker")
        import torch
        model, fit = plda_mod.fit(dz.eng, got["E"], torch.from_numpy(labels).to(got["E"].device), D0, lda_dim, n_iters, K=len(keys))
        report = {"rows_used": int(len(labels)), "rows_dropped": int(got["n_dropped"]), "classes": int(fit.n_classes), "class_keys": keys,
                  "counts": fit.counts, "objf": fit.objf}
        if out_dir is not None:
            out = Path(out_dir)
            out.mkdir(parents=True, exist_ok=True)
            report["transform_npz"], report["plda_npz"] = out / "xvec_transform.npz", out / "plda.npz"
            plda_mod.save_plda(model, report["transform_npz"], report["plda_npz"])
        return model, report

    def open_streams(self, n_streams: int = 1, **options):
        """Streaming diarization: a stream.StreamBank of n_streams live streams on the models diarize loads (options: step_s, latency_s,
        capacity, delta_new, max_speakers).  bank.push([samples or None per stream]) feeds 16 kHz mono int16 audio as it arrives and returns
        the newly emitted frames per stream, bank.finish(r) ends a stream with its diarize.DiarizationResult (stream.py states the rule).
        The bank steps in the ResNet34's numerical contract; every push and finish gives the engine back in the precision it had."""
        return self.diarizer().open_streams(n_streams, **options)

    def link_speakers(self, results, threshold: float = 0.7045654963945799, min_speech_s: float = 0.0, candidates=None):
        """One speaker inventory for the results of diarize_many (diarize.link_speakers, which states the rule): the local speakers of
        different recordings joined into global ones by a constrained centroid linkage on the device - two speakers of one recording never
        join - cut at `threshold` (PyAnnote's within-recording default: untuned for centroids across recordings, pass your own).
        candidates: profile dicts as identify_speaker takes them, loaded through the same store path; each enrolled speaker gives ONE row, the
        float64 mean of their enrolled unit embeddings, re-normalised, and no global speaker ever holds two of them.  The result
        (diarize.SpeakerLinks) then carries names [n_global]: the speaker_id, or None.  The centroids of a diarization live in the
        diarizer's space, so candidates need it to be the enrolled one: SDK_MODEL=resnet34, or SDK_MODEL=ecapa with SDK_DIARIZE_MODEL=ecapa."""
        if self.lite:
            raise ValueError("link_speakers needs the torch engine: not available with SDK_NO_TORCH=1")
        if candidates is not None and not (self.model == "resnet34" or (self.model == "ecapa" and self.diarize_model == "ecapa")):
            raise ValueError(f"link_speakers: candidates are enrolled in the {self.model!r} embedding space (SDK_MODEL), the centroids of a diarization "
                             f"in the diarizer's {self.diarize_model!r} space (SDK_DIARIZE_MODEL): enrol and link with SDK_MODEL=resnet34, or with "
                             "SDK_MODEL=ecapa and SDK_DIARIZE_MODEL=ecapa")
        from .diarize import link_speakers
        profiles, names = None, None
        if candidates is not None:
            batch = self._load_candidates(candidates)
            names = list(dict.fromkeys(batch.speaker_ids))                       # one row per speaker, in order of first appearance
            M = np.asarray(batch.matrix, dtype=np.float64).reshape(len(batch), -1)
            M = M / np.maximum(np.linalg.norm(M, axis=1, keepdims=True), 1e-12)
            sid = np.asarray([names.index(s) for s in batch.speaker_ids], dtype=np.int64)
            mean = np.stack([M[sid == i].mean(axis=0) for i in range(len(names))]) if names else np.zeros((0, int(self.embedding_dim)))
            profiles = (mean / np.maximum(np.linalg.norm(mean, axis=1, keepdims=True), 1e-12)).astype(np.float32)
        links = link_speakers(self.engine(), results, threshold, min_speech_s, profiles)
        if names is not None:
            links.names = [names[p] if p >= 0 else None for p in links.profile.tolist()]
        return links

    # ---- a2: enroll (base.py:107-128) ---------------------------------------------------------
    def _enroll_vector(self, audio_path: Path, segments: Optional[List[Tuple[float, float]]] = None):
        """The unit mean embedding of a recording's windows (what enroll_speaker stores) and the windows' spans."""
        if segments:           # the caller vouches that each range is this speaker: true-length windows, never widened
            samples = decode_to_profile(Path(audio_path), self.engine(), self.get_audio_profile())
            if self.lite:
                starts_by, wins, _ = range_starts(len(samples), list(segments), hop_s=self.hop_s)
                parts = self.embed_tables_host(samples, starts_by) if wins else {}
                spans = [(ri, a, b) for ri, _, _, a, b in wins]
                E = np.stack([parts[S][0][row] for _, S, row, _, _ in wins]) if wins else None
            else:
                E, _, _, spans, _ = self.embed_ranges(samples, list(segments))
            if not spans:
                raise ValueError(f"{audio_path}: no analysable audio (every segment shorter than 0.5 s)")
        else:
            samples, starts, W, spans = self._windows(audio_path, None)
            E = self.embed_tables_host(samples, {W: starts})[W][0] if self.lite else self.embed_tables(samples, {W: starts})[W][0]
        if self.lite:
            mean = E.astype(np.float64).mean(axis=0)
            vec = (mean / max(float(np.linalg.norm(mean)), 1e-12)).astype(np.float32)
        else:
            mean = E.double().mean(dim=0)
            vec = (mean / mean.norm().clamp_min(1e-12)).float().cpu().numpy()
        return vec, spans

    def enroll_speaker(self, audio_path: Path, segments: Optional[List[Tuple[float, float]]] = None) -> Dict[str, Any]:
        vec, spans = self._enroll_vector(audio_path, segments)
        ext = save_vector(vec, meta=self.numerics())
        return {
            "external_id": ext,                      # the only backend field cmd_enroll persists (speaker_detection:890-904)
            "file": str(vector_path(ext)),
            "model_version": self.model_version,
            "source_audio": str(audio_path),
            "source_segments": segments,
            "embedding_dim": self.embedding_dim,
            "n_windows": len(spans),
        }

    # ---- a1: identify (base.py:130-151) --------------------------------------------------------
    def profile_tensors(self, batch):
        """Device copies (unit rows fp32, bf16, max rounding residual) of a ProfileBatch, made once per batch object.  Pack hit: the three arrays
        are uploaded as sdk_l2norm wrote them when the pack was built (no per-embedding file I/O happened, no normalisation pass runs).  Pack
        miss: one sdk_l2norm pass, whose outputs are then published as the set's pack (store.publish_pack) - so hit and miss score bit-identically."""
        import torch
        eng = self.engine()

        def make():
            if batch.norm is not None:
                E, Eb, r = batch.norm
                Pn = torch.from_numpy(np.array(E, dtype=np.float32)).to(eng.device)
                Pb = torch.from_numpy(np.array(Eb, dtype=np.uint16).view(np.int16)).to(eng.device).view(torch.bfloat16)
                rp = torch.from_numpy(np.array(r, dtype=np.float32)).to(eng.device)
            else:
                Pn, Pb, rp = eng.l2norm(torch.from_numpy(np.ascontiguousarray(batch.matrix, dtype=np.float32)).to(eng.device))
                if batch.pack_ref:
                    publish_pack(batch, Pn.cpu().numpy(), Pb.view(torch.int16).cpu().numpy().view(np.uint16), rp.cpu().numpy())
            return Pn, Pb, rp.max().reshape(1)
        return cached(batch, "_dev", eng, None, make)

    # ---- adaptive score normalisation (snorm.py) ---------------------------------------------------
    def make_cohort(self, audio_paths: List[Path], out_path: Path) -> Dict[str, Any]:
        """One row per recording - the unit mean embedding enroll_speaker would store for it - written as a [M, d] fp32 .npy: the file
        SDK_COHORT names.  The recordings should be speakers that are NOT among the enrolled ones (impostors)."""
        rows = [self._enroll_vector(Path(p), None)[0] for p in audio_paths]
        if not rows:
            raise ValueError("make_cohort: no recordings")
        mat = np.ascontiguousarray(np.stack(rows), dtype=np.float32)
        out_path = Path(out_path)
        with open(out_path, "wb") as f:                 # an open file: np.save appends no suffix of its own
            np.save(f, mat, allow_pickle=False)
        return {"file": str(out_path), "n_recordings": int(mat.shape[0]), "embedding_dim": int(mat.shape[1]), "model_version": self.model_version}

    def cohort(self):
        """The configured snorm.Cohort (None without SDK_COHORT), loaded on first use."""
        return self.rule.cohort(self)

    def profile_stats(self, batch):
        """(mean_p, std_p) device tensors: the cohort statistics of a ProfileBatch's rows, computed once per batch object and cached on it
        beside its device copies, keyed by the cohort's digest and K."""
        eng, co = self.engine(), self.cohort()
        K = min(self.cohort_topk, len(co))
        return cached(batch, "_snorm", eng, (co.digest, K), lambda: eng.cohort_stats(self.profile_tensors(batch)[0], co.device_rows(eng), K))

    def score_windows_snorm(self, E, batch, k: int = 1):
        """score_windows on the normalised scale -> (idx, z, raw) on the host; needs a configured cohort."""
        if self.cohort() is None:
            raise ValueError("score_windows_snorm: no cohort configured (SDK_COHORT)")
        return tuple(t.cpu().numpy() for t in self.rule.enqueue(self, (E, None, None), batch, k))

    # ---- PLDA log-likelihood-ratio scoring (plda_score.py) ------------------------------------------------
    @property
    def plda_scoring(self) -> bool:
        """Whether identify / verify decide on the PLDA log-likelihood ratio (SDK_SCORE_PLDA_TRANSFORM and SDK_SCORE_PLDA are set)."""
        return self.score_plda_paths is not None

    def score_plda(self):
        """The configured scoring model (plda.Plda; None without SDK_SCORE_PLDA*), loaded on first use.  A model whose d_in is not this
        family's embedding_dim is refused."""
        return self.rule.model(self)

    def _plda_rows(self, E):
        """fp32 unit rows [n, d] (device) -> their float64 rows [n, D] in the scoring model's space (plda_transform, 65 536 rows per call)."""
        import torch
        eng, model = self.engine(), self.score_plda()
        E = E.contiguous()
        n, step = int(E.shape[0]), 65536
        if n == 0:
            return torch.empty((0, model.lda_dim), dtype=torch.float64, device=E.device)
        parts = [eng.plda_transform(E, torch.arange(a, min(n, a + step), dtype=torch.int32, device=E.device), model, check_rows=False)
                 for a in range(0, n, step)]
        return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)

    def speaker_table(self, batch):
        """The speaker table of a ProfileBatch under the scoring model -> (G, r device tensors, speakers, first rows, counts): its rows
        grouped by speaker_id (plda_score.group_speakers), transformed and pooled on the device (Engine.plda_enroll), computed once per batch
        object and cached on it, keyed by the model's content digest and the count mode."""
        import torch
        from .plda_score import group_speakers
        eng, model = self.engine(), self.score_plda()

        def make():
            group, speakers, first, counts = group_speakers(batch.speaker_ids)
            n_eff = counts.astype(np.float64) if self.score_plda_count else np.ones(len(speakers), np.float64)
            Xp = self._plda_rows(self.profile_tensors(batch)[0])
            G, r, _ = eng.plda_enroll(Xp, torch.from_numpy(group).to(eng.device), torch.from_numpy(n_eff).to(eng.device),
                                      model.device_arrays(eng.device)["Phi"])          # group_speakers' labels lie in [0, S): status is not read
            return G, r, speakers, first, counts
        return cached(batch, "_plda", eng, (self._score_plda[1], self.score_plda_count), make)

    def score_windows_plda(self, E, batch, k: int = 1):
        """score_windows on the PLDA scale: E [N, d] fp32 unit rows (device) -> (idx [N, k] int32: SPEAKER indices in the order of
        plda_score.group_speakers(batch.speaker_ids), llr [N, k] float64) on the host; needs a configured scoring model."""
        if self.score_plda() is None:
            raise ValueError("score_windows_plda: no scoring model configured (SDK_SCORE_PLDA_TRANSFORM and SDK_SCORE_PLDA)")
        return tuple(t.cpu().numpy() for t in self.rule.enqueue(self, (E, None, None), batch, k))

    def score_windows(self, E, Eb, re, batch, k: int = 1):
        """Device scoring of embedded windows against a ProfileBatch -> (idx, score) on host: cosines, whatever the Backend's rule is."""
        idx, sc = Cosine().enqueue(self, (E, Eb, re), batch, k)
        return idx.cpu().numpy(), sc.cpu().numpy()

    def _load_candidates(self, candidates: List[Dict[str, Any]]):
        """The candidate set as one ProfileBatch (pack hit or file by file), with everything a user must hear about it on stderr."""
        batch = self.last_batch = load_profile_batch(candidates, self.name, model_prefix=f"{self.name}-", model_version=self.model_version,
                                                     settings=self.numerics())
        for why in batch.skipped:
            print(f"mi355x backend: skipped embedding {why}", file=sys.stderr)
        for why in batch.warnings[:5]:
            print(f"mi355x backend: warning: {why}", file=sys.stderr)
        if len(batch.warnings) > 5:
            print(f"mi355x backend: warning: ... and {len(batch.warnings) - 5} more embeddings enrolled under another numerical setting", file=sys.stderr)
        if batch.all_skipped_message():
            # candidates exist but none is comparable: "no match" would be a lie.  The CLI prints "Error during identification: ..."
            # and exits 1 (speaker_detection:1072-1074); speaker-assign then records no embedding signal (speaker-assign:296)
            raise ValueError(batch.all_skipped_message())
        return batch

    def _enqueue_identify(self, audio_path: Path, batch):
        """One recording on the torch engine: its windows embedded and the rule's top-1 against the batch enqueued -> (device columns, spans).
        Nothing waits on the host here."""
        samples, starts, W, spans = self._windows(audio_path, None)
        return self.rule.enqueue(self, self.embed_tables(samples, {W: starts})[W], batch), spans

    def _collect_identify(self, pending, batch, threshold: float) -> List[Dict[str, Any]]:
        """The result rows of one _enqueue_identify: its columns downloaded (the host waits here) and aggregated by the rule."""
        cols, spans = pending
        return self.rule.rows(self, [t.cpu().numpy()[:, 0] for t in cols], spans, batch, threshold)

    def _identify_lite(self, audio_path: Path, batch, threshold: float) -> List[Dict[str, Any]]:
        """One recording on the torch-free path (SDK_NO_TORCH=1; the cosine rule only): embedded, scored and downloaded on the null stream."""
        samples, starts, W, spans = self._windows(audio_path, None)
        _, idx, sc = self.embed_tables_host(samples, {W: starts}, batch)[W]
        return self.rule.rows(self, (idx[:, 0], sc[:, 0]), spans, batch, threshold)      # the cosine rule's rows, calibration included

    def identify_speaker(self, audio_path: Path, candidates: List[Dict[str, Any]], threshold: float = 0.354) -> List[Dict[str, Any]]:
        """With a cohort configured (SDK_COHORT) a window's winner is its normalised top-1 and it votes when z >= SDK_COHORT_THRESHOLD: the raw
        `threshold` is NOT applied.  The rows then carry norm_score and are sorted by it (aggregate_matches_snorm).
        With a scoring PLDA configured (SDK_SCORE_PLDA*) a window's winner is the SPEAKER of its largest log-likelihood ratio and it votes
        when llr >= SDK_SCORE_PLDA_THRESHOLD: the raw `threshold` is NOT applied.  The rows then carry llr (uncalibrated) and n_embeddings,
        similarity = confidence = 1 / (1 + exp(-llr)), embedding_id is the speaker's first embedding, and they are sorted by llr
        (plda_score.aggregate_matches_plda)."""
        batch = self._load_candidates(candidates)
        if len(batch) == 0:
            return []
        if self.lite:
            return self._identify_lite(audio_path, batch, threshold)
        return self._collect_identify(self._enqueue_identify(audio_path, batch), batch, threshold)

    def identify_many(self, audio_paths: List[Path], candidates: List[Dict[str, Any]], threshold: float = 0.354) -> List[List[Dict[str, Any]]]:
        """identify_speaker over SEVERAL recordings against one candidate set, as one pipelined pass (an extension: the reference's contract is one
        recording per call, base.py:130-151, and gets its concurrency from up to four CLI processes, speaker-process:627-629).  The profiles are
        loaded and uploaded once; every recording is decoded, handed to the staging slots and its kernels enqueued WITHOUT waiting for the previous
        one - the upload of recording i + 1 runs under the forward pass of recording i (csrc/ingest.hip) - and the host synchronises once, at the end.
        Row lists equal identify_speaker's, recording by recording (tests/test_gpu_ingest.py).  With a cohort configured (SDK_COHORT) the
        decision is identify_speaker's normalised one and the raw `threshold` is NOT applied; with a scoring PLDA (SDK_SCORE_PLDA*) it is
        identify_speaker's log-likelihood-ratio one, and the raw `threshold` is NOT applied either."""
        batch = self._load_candidates(candidates)
        if len(batch) == 0:
            return [[] for _ in audio_paths]
        if self.lite:                       # the torch-free path downloads per recording (everything on the null stream): sequential
            return [self._identify_lite(path, batch, threshold) for path in audio_paths]
        pending = [self._enqueue_identify(path, batch) for path in audio_paths]             # enqueued; nothing waits here
        return [self._collect_identify(p, batch, threshold) for p in pending]

    # ---- a3: verify - the CLI reads result['confidence'] (speaker_detection:1173-1174) ---------
    def verify_speaker(self, audio_path: Path, speaker_profile: Dict[str, Any], threshold: float = 0.354) -> Dict[str, Any]:
        """With a cohort configured (SDK_COHORT) the match is identify_speaker's normalised decision (the raw `threshold` is NOT applied) and
        the result carries norm_score; similarity and confidence stay the mean raw cosine.  With a scoring PLDA configured (SDK_SCORE_PLDA*)
        the match is identify_speaker's log-likelihood-ratio decision (the raw `threshold` is NOT applied), the result carries llr, and
        similarity and confidence are 1 / (1 + exp(-llr))."""
        hits = self.identify_speaker(audio_path, [speaker_profile], threshold)
        if not hits:
            return {"match": False, "similarity": 0.0, "confidence": 0.0, "embedding_id": None}
        h = hits[0]
        out = {"match": True, "similarity": h["similarity"], "confidence": h["similarity"], "embedding_id": h.get("embedding_id")}
        out.update((key, h[key]) for key in self.rule.verify_keys)          # norm_score under a cohort, llr under a scoring PLDA
        return out
