"""The decision rule of identify_speaker, identify_many, verify_speaker and score_verification: ONE of three, chosen by the environment
(rule_from_env; backend.py's docstring states the variables).

  Cosine   the raw cosine of a window against its best enrolled embedding, voting at the caller's `threshold`
  Snorm    the cohort-normalised z of snorm.py (SDK_COHORT*), voting at SDK_COHORT_THRESHOLD
  Plda     the log-likelihood ratio of plda_score.py against an enrolled SPEAKER (SDK_SCORE_PLDA*), voting at SDK_SCORE_PLDA_THRESHOLD

A rule holds its settings and its lazily loaded model (cohort(be) / model(be)) and answers, for the Backend `be` that owns it:

  enqueue(be, (E, Eb, resid), batch, k)   the device tensors of the top-k of embedded windows against a ProfileBatch; nothing waits
  rows(be, columns, spans, batch, threshold)   the result rows from the downloaded top-1 columns (in enqueue's order)
  refuse_trials() / trial_matrices(be, E, batch)   what score_verification scores
  verify_keys   the keys of a result row that verify_speaker copies beside the ABC's own
  calibrated(rows, key)   with SDK_SCORE_CALIBRATION: the rows with calibrated_llr and posterior added (below); else the rows as they are

The Backend keeps what is per candidate set and cached on it (profile_tensors, profile_stats, speaker_table; `cached` below is their one
cache) and the public score_windows* calls.  This module imports neither torch nor the engine until a rule computes.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import numpy as np


def cached(batch, slot: str, eng, key, make):
    """make(), computed once per batch object, engine and key: kept on the batch as `slot` = (eng, key, value)."""
    got = getattr(batch, slot, None)
    if got is None or got[0] is not eng or got[1] != key:
        got = (eng, key, make())
        setattr(batch, slot, got)
    return got[2]


# ---- votes -> result rows ---------------------------------------------------------------------------------------------------------------
def _tally(votes, spans) -> Dict[Any, Dict[str, Any]]:
    """The voting loop of the three aggregations.  votes: per window None (it does not vote) or (key, value) -> {key: {"votes": the values
    of its voting windows, "first": the start of its first, "last": the end of its last}}, keys in order of their first vote."""
    per: Dict[Any, Dict[str, Any]] = {}
    for w, vote in enumerate(votes):
        if vote is None:
            continue
        acc = per.setdefault(vote[0], {"votes": [], "first": spans[w][0], "last": spans[w][1]})
        acc["votes"].append(vote[1])
        acc["last"] = spans[w][1]
    return per


def _mean(values) -> float:
    return float(np.mean(np.asarray(values, dtype=np.float64)))


def _winner(rows) -> int:
    """The profile row that won most windows (ties: the first row)."""
    return max(set(rows), key=lambda row: (rows.count(row), -row))


def aggregate_matches(best_idx: np.ndarray, best_score: np.ndarray, spans, batch, threshold: float) -> List[Dict[str, Any]]:
    """Per-window argmax (integer profile row, fp32 cosine) -> one result row per matched speaker.
    A window votes for the speaker owning its best profile row if the cosine clears `threshold`;
    similarity = float64 mean of the speaker's window scores; rows sorted by similarity desc, ties
    by speaker id.  embedding_id = the speaker's embedding that won most windows (ties: first)."""
    per = _tally((None if row < 0 or s < threshold else (batch.speaker_ids[row], (row, float(s)))
                  for row, s in zip(best_idx.tolist(), best_score.tolist())), spans)
    out = []
    for sid, acc in per.items():
        rows, scores = zip(*acc["votes"])
        sim = _mean(scores)
        out.append({"speaker_id": sid, "similarity": sim, "confidence": sim, "embedding_id": batch.embedding_ids[_winner(rows)],
                    "segment": (acc["first"], acc["last"]), "n_segments": len(scores)})
    out.sort(key=lambda r: (-r["similarity"], r["speaker_id"]))
    return out


def aggregate_matches_snorm(best_idx: np.ndarray, best_z: np.ndarray, best_raw: np.ndarray, spans, batch, z_threshold: float) -> List[Dict[str, Any]]:
    """aggregate_matches for the normalised path (snorm.py): a window votes for the speaker owning its normalised top-1 row when its z clears
    `z_threshold` (no raw threshold applies).  similarity = confidence = float64 mean of the RAW cosines of the speaker's voting windows (so
    combine_signals keeps its [-1, 1] input); norm_score = float64 mean of their z.  Rows sorted by norm_score descending, then speaker id."""
    per = _tally((None if row < 0 or not z >= z_threshold else (batch.speaker_ids[row], (row, float(z), float(s)))
                  for row, z, s in zip(best_idx.tolist(), best_z.tolist(), best_raw.tolist())), spans)
    out = []
    for sid, acc in per.items():
        rows, zs, raws = zip(*acc["votes"])
        sim = _mean(raws)
        out.append({"speaker_id": sid, "similarity": sim, "confidence": sim, "norm_score": _mean(zs), "embedding_id": batch.embedding_ids[_winner(rows)],
                    "segment": (acc["first"], acc["last"]), "n_segments": len(zs)})
    out.sort(key=lambda r: (-r["norm_score"], r["speaker_id"]))
    return out


# ---- the rules ----------------------------------------------------------------------------------------------------------------------------
class Rule:
    """What the three rules share: the settings of the other two at their unconfigured values (the Backend's attributes of the same names
    read them) and no lazily loaded state."""
    verify_keys = ()
    cohort_path: Optional[str] = None
    cohort_threshold: Optional[float] = None
    cohort_topk = 300
    score_plda_paths = None
    score_plda_dim, score_plda_threshold, score_plda_count = 128, 0.0, True
    loaded = None                                   # Plda: (plda.Plda, content digest) once model(be) has read the files
    calibration = None                              # trials.Calibration of SDK_SCORE_CALIBRATION
    score_prior = 0.5                               # SDK_SCORE_PRIOR

    def cohort(self, be):
        return None

    def model(self, be):
        return None

    def refuse_trials(self) -> None:
        """Raise where score_verification has no matrix form of this rule; before it does any work."""

    def calibrated(self, rows, key: str):
        """With a calibration configured every row gains calibrated_llr = a * row[key] + b in float64 and
        posterior = sigmoid(calibrated_llr + logit(score_prior)); nothing else changes - no decision, threshold, order or existing key.
        row[key] is the mean score of the speaker's voting windows (the cosine, or the llr under PLDA); an affine map commutes with the
        mean, so calibrated_llr is the mean of the windows' calibrated log-likelihood ratios.  Without one the rows are returned as they
        are."""
        cal = self.calibration
        if cal is None:
            return rows
        shift = float(np.log(self.score_prior / (1.0 - self.score_prior)))
        for row in rows:
            llr = float(cal.llr(row[key]))
            x = llr + shift
            row["calibrated_llr"] = llr
            row["posterior"] = float(1.0 / (1.0 + np.exp(-x))) if x >= 0 else float(np.exp(x) / (1.0 + np.exp(x)))
        return rows


class Cosine(Rule):
    kind = "cosine"

    def enqueue(self, be, emb, batch, k: int = 1):
        """-> (idx, cosine)"""
        Pn, Pb, rpm = be.profile_tensors(batch)
        return be.engine().affinity_topk(*emb, Pn, Pb, rpm, k=min(k, len(batch)))

    def rows(self, be, cols, spans, batch, threshold: float):
        return self.calibrated(aggregate_matches(cols[0], cols[1], spans, batch, threshold), "similarity")

    def trial_matrices(self, be, E, batch):
        """Test rows E against the candidates' enrolled embeddings -> (A, B, r, the label of every model row, kind, {speaker id: label})."""
        import torch
        index: Dict[Any, int] = {}
        for sid in batch.speaker_ids:
            index.setdefault(sid, len(index))
        A, B = E.double(), be.profile_tensors(batch)[0].double().contiguous()
        return A, B, torch.zeros((int(B.shape[0]),), dtype=torch.float64, device=E.device), [index[sid] for sid in batch.speaker_ids], self.kind, index


class Snorm(Rule):
    kind = "snorm"
    verify_keys = ("norm_score",)

    def __init__(self, path: str, threshold: float) -> None:
        self.cohort_path, self.cohort_threshold = path, threshold
        self._cohort = None

    def cohort(self, be):
        """The snorm.Cohort, loaded on first use."""
        if self._cohort is None:
            from .snorm import Cohort
            self._cohort = Cohort.load(self.cohort_path, be.embedding_dim)
        return self._cohort

    def enqueue(self, be, emb, batch, k: int = 1):
        """-> (idx, z, raw cosine)"""
        eng, co = be.engine(), self.cohort(be)
        mean_p, std_p = be.profile_stats(batch)
        mean_e, std_e = eng.cohort_stats(emb[0], co.device_rows(eng), min(self.cohort_topk, len(co)))
        return eng.affinity_topk_snorm(emb[0], mean_e, std_e, be.profile_tensors(batch)[0], mean_p, std_p, k=max(1, min(k, len(batch), 4)))

    def rows(self, be, cols, spans, batch, threshold: float):
        return aggregate_matches_snorm(cols[0], cols[1], cols[2], spans, batch, self.cohort_threshold)

    def refuse_trials(self) -> None:
        raise ValueError("score_verification: AS-norm trials are not built: with SDK_COHORT set the decision is made on the normalised scale, "
                         "which has no matrix form here; unset SDK_COHORT to evaluate the cosine or the PLDA rule.  The normalised scale "
                         "has entry points of its own: backend.score_verification_snorm(backend, ...) and "
                         "backend.tune_cohort_threshold(backend, ...) (trials_snorm.py)")


class Plda(Rule):
    kind = "plda"
    verify_keys = ("llr",)

    def __init__(self, paths, dim: int, threshold: float, count: bool) -> None:
        self.score_plda_paths, self.score_plda_dim, self.score_plda_threshold, self.score_plda_count = paths, dim, threshold, count

    def model(self, be):
        """The plda.Plda, loaded on first use.  A model whose d_in is not the family's embedding_dim is refused."""
        if self.loaded is None:
            import hashlib
            from .plda import load_plda
            model = load_plda(self.score_plda_paths[0], self.score_plda_paths[1], self.score_plda_dim)
            if model.d_in != int(be.embedding_dim):
                raise ValueError(f"SDK_SCORE_PLDA_TRANSFORM={self.score_plda_paths[0]}: the PLDA model takes d_in={model.d_in}, the {be.model!r} family "
                                 f"(SDK_MODEL) embeds into embedding_dim={int(be.embedding_dim)}: train one in this space (Backend.train_plda)")
            h = hashlib.sha256(np.asarray([model.lda_dim], dtype=np.int64).tobytes())
            for a in (model.mean1, model.lda, model.mean2, model.mu, model.tr, model.psi):
                h.update(np.asarray(a.shape, dtype=np.int64).tobytes())
                h.update(a.tobytes())
            self.loaded = (model, h.hexdigest()[:16])
        return self.loaded[0]

    def enqueue(self, be, emb, batch, k: int = 1):
        """-> (idx: SPEAKER indices in the order of plda_score.group_speakers(batch.speaker_ids), llr)"""
        import torch
        eng = be.engine()
        G, r = be.speaker_table(batch)[:2]
        X = be._plda_rows(emb[0])
        k = max(1, min(int(k), int(G.shape[0]), 4))
        n, step = int(X.shape[0]), 65536
        if n <= step:
            return eng.plda_score_topk(X, G, r, k=k)
        parts = [eng.plda_score_topk(X[a:a + step], G, r, k=k) for a in range(0, n, step)]
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])

    def rows(self, be, cols, spans, batch, threshold: float):
        from .plda_score import aggregate_matches_plda
        _, _, speakers, first, counts = be.speaker_table(batch)
        return self.calibrated(aggregate_matches_plda(cols[0], cols[1], spans, speakers, [batch.embedding_ids[int(p)] for p in first], counts,
                                                      self.score_plda_threshold), "llr")

    def trial_matrices(self, be, E, batch):
        """Test rows E against the candidates' SPEAKERS (speaker_table) -> (A, B, r, the label of every model row, kind, {speaker id: label})."""
        import torch
        G, r, speakers = be.speaker_table(batch)[:3]
        X = be._plda_rows(E)
        return torch.cat([X, X * X], dim=1).contiguous(), G, r, np.arange(len(speakers)), self.kind, {sid: s for s, sid in enumerate(speakers)}


def rule_from_env(environ) -> Rule:
    """The configured rule, or the refusal of a setting that does not hold together.  Reads no file but the calibration's
    (SDK_SCORE_CALIBRATION: a few hundred bytes of JSON, whose kind must be the rule's)."""
    lite = environ.get("SDK_NO_TORCH") == "1"
    # adaptive score normalisation (snorm.py): off unless a cohort is configured
    cohort, topk, thr = environ.get("SDK_COHORT") or None, int(environ.get("SDK_COHORT_TOPK", "300")), environ.get("SDK_COHORT_THRESHOLD")
    rule: Rule = Cosine()
    if bool(cohort) != bool(thr):
        raise ValueError("SDK_COHORT (the cohort file) and SDK_COHORT_THRESHOLD (the vote threshold on the normalised scale) go together: "
                         f"{'SDK_COHORT_THRESHOLD' if cohort else 'SDK_COHORT'} is not set.  There is no default threshold: it depends on "
                         "the model family and the cohort")
    if cohort:
        try:
            rule = Snorm(cohort, float(thr))
        except ValueError:
            raise ValueError(f"SDK_COHORT_THRESHOLD={thr!r}: a float on the normalised (z) scale expected") from None
        if rule.cohort_threshold != rule.cohort_threshold:
            raise ValueError("SDK_COHORT_THRESHOLD is NaN: a float on the normalised (z) scale expected")
        if topk < 1:
            raise ValueError(f"SDK_COHORT_TOPK={topk}: at least 1")
        if lite:
            raise ValueError("SDK_COHORT with SDK_NO_TORCH=1: the normalised path needs the torch engine; unset SDK_NO_TORCH (or SDK_COHORT)")
    # PLDA log-likelihood-ratio scoring (plda_score.py): off unless a scoring model is configured
    tpath, ppath = environ.get("SDK_SCORE_PLDA_TRANSFORM") or None, environ.get("SDK_SCORE_PLDA") or None
    if bool(tpath) != bool(ppath):
        raise ValueError("SDK_SCORE_PLDA_TRANSFORM and SDK_SCORE_PLDA name the two files of one PLDA model: set both or neither "
                         f"({'SDK_SCORE_PLDA' if tpath else 'SDK_SCORE_PLDA_TRANSFORM'} is not set)")
    if tpath:
        if cohort:
            raise ValueError("SDK_SCORE_PLDA* together with SDK_COHORT: the identify decision is made on ONE scale, the PLDA log-likelihood "
                             "ratio or the cohort-normalised cosine; unset one of them")
        if lite:
            raise ValueError("SDK_SCORE_PLDA* with SDK_NO_TORCH=1: PLDA scoring needs the torch engine; unset SDK_NO_TORCH (or SDK_SCORE_PLDA*)")
        dim = environ.get("SDK_SCORE_PLDA_DIM", "128").strip()
        if dim not in ("64", "128"):
            raise ValueError(f"SDK_SCORE_PLDA_DIM={dim!r}: the PLDA dimensions kept, 64 or 128")
        thr = environ.get("SDK_SCORE_PLDA_THRESHOLD", "0")
        try:
            llr = float(thr)
        except ValueError:
            raise ValueError(f"SDK_SCORE_PLDA_THRESHOLD={thr!r}: a float on the log-likelihood-ratio scale expected") from None
        if llr != llr:
            raise ValueError("SDK_SCORE_PLDA_THRESHOLD is NaN: a float on the log-likelihood-ratio scale expected")
        cnt = environ.get("SDK_SCORE_PLDA_COUNT", "1").strip()
        if cnt not in ("0", "1"):
            raise ValueError(f"SDK_SCORE_PLDA_COUNT={cnt!r}: 1 (a speaker's count is the number of their enrolled embeddings) or 0 (it is 1)")
        rule = Plda((tpath, ppath), int(dim), llr, cnt == "1")
    rule.cohort_topk = topk
    # the calibration of the rule's score (trials.py): off unless a file is configured
    cpath = environ.get("SDK_SCORE_CALIBRATION") or None
    if cpath:
        if cohort:
            raise ValueError("SDK_SCORE_CALIBRATION together with SDK_COHORT: calibrations are fitted to the cosine or the PLDA rule "
                             "(backend.calibrate_verification(backend, ...) refuses a cohort); unset one of them")
        prior = environ.get("SDK_SCORE_PRIOR", "0.5")
        try:
            rule.score_prior = float(prior)
        except ValueError:
            raise ValueError(f"SDK_SCORE_PRIOR={prior!r}: the prior of a target, a float inside (0, 1)") from None
        if not 0.0 < rule.score_prior < 1.0:
            raise ValueError(f"SDK_SCORE_PRIOR={prior!r}: the prior of a target, a float inside (0, 1)")
        from .trials import load_calibration
        cal = load_calibration(cpath)
        if cal.kind != rule.kind:
            raise ValueError(f"SDK_SCORE_CALIBRATION={cpath}: fitted to the {cal.kind!r} rule, the configured rule is {rule.kind!r}: "
                             "calibrate under the settings you score with (backend.calibrate_verification(backend, ...))")
        rule.calibration = cal
        rule.verify_keys = tuple(rule.verify_keys) + ("calibrated_llr", "posterior")
    return rule
