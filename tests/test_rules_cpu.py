"""CPU checks of the decision rules (rules.py) and of the Backend that dispatches to them: the Backend's public surface is the one it had
while the three rules were if-chains in backend.py, importing it stays torch-free, the three aggregations answer what they answered before
they shared one voting loop (tests/golden/aggregate_rows.json), identify_many enqueues every recording before it downloads anything, and
the configuration refusals come in the order they came in."""
from __future__ import annotations

import inspect
import json
import subprocess
import sys

import numpy as np
import pytest
from conftest import GOLDEN, PKG, ROOT, sub

BK = sub("backend")
RULES = sub("rules")
PS = sub("plda_score")

# every public attribute of the Backend class (and _plda_rows, which tests call) before rules.py: name -> str(inspect.signature(...)), or "property"
PUBLIC = {
    '_plda_rows': '(self, E)',
    'audio_profile': 'property',
    'check_embedding_compatibility': "(self, embedding: 'Dict[str, Any]') -> 'Dict[str, Any]'",
    'cluster_ranges': "(self, samples: 'np.ndarray', ranges: 'List[Tuple[float, float]]', threshold: 'float' = 0.7045654963945799, min_cluster_size: 'int' = 12, speakers=None, clustering: 'str' = 'ahc', loop_prob: 'float' = 0.99, plda=None)",
    'cohort': '(self)',
    'diarize': '(self, samples_or_path, **kw)',
    'diarize_many': '(self, samples_or_paths, **kw)',
    'diarizer': '(self)',
    'embed_ranges': "(self, samples: 'np.ndarray', ranges: 'List[Tuple[float, float]]')",
    'embed_tables': "(self, samples: 'np.ndarray', tables: 'Dict[int, np.ndarray]')",
    'embed_tables_host': "(self, samples: 'np.ndarray', tables: 'Dict[int, np.ndarray]', batch=None, k: 'int' = 1)",
    'embed_windows': "(self, pcm: 'np.ndarray')",
    'embed_windows_host': "(self, pcm: 'np.ndarray', profiles=None, k: 'int' = 1)",
    'embedding_dim': 'property',
    'engine': '(self)',
    'enroll_speaker': "(self, audio_path: 'Path', segments: 'Optional[List[Tuple[float, float]]]' = None) -> 'Dict[str, Any]'",
    'extract_segments_from_transcript': "(self, transcript_path: 'Path', speaker_label: 'str') -> 'List[Tuple[float, float]]'",
    'get_audio_profile': "(self) -> 'AudioProfile'",
    'identify_many': "(self, audio_paths: 'List[Path]', candidates: 'List[Dict[str, Any]]', threshold: 'float' = 0.354) -> 'List[List[Dict[str, Any]]]'",
    'identify_speaker': "(self, audio_path: 'Path', candidates: 'List[Dict[str, Any]]', threshold: 'float' = 0.354) -> 'List[Dict[str, Any]]'",
    'link_speakers': "(self, results, threshold: 'float' = 0.7045654963945799, min_speech_s: 'float' = 0.0, candidates=None)",
    'lite': 'property',
    'make_cohort': "(self, audio_paths: 'List[Path]', out_path: 'Path') -> 'Dict[str, Any]'",
    'model_version': 'property',
    'name': 'property',
    'numerics': "(self) -> 'Dict[str, Any]'",
    'open_streams': "(self, n_streams: 'int' = 1, **options)",
    'plda_scoring': 'property',
    'profile_stats': '(self, batch)',
    'profile_tensors': '(self, batch)',
    'requires_api_key': 'property',
    'score_diarization': "(self, results, references, uris=None, collar_s: 'float' = 0.0, skip_overlap: 'bool' = False)",
    'score_plda': '(self)',
    'score_ranges': "(self, samples: 'np.ndarray', ranges: 'List[Tuple[float, float]]', batch, k: 'int' = 1)",
    'score_verification': "(self, audio_paths, speaker_ids, candidates, score_range=None, p_target: 'float' = 0.01, c_miss: 'float' = 1.0, c_fa: 'float' = 1.0, max_refine: 'int' = 8)",
    'score_windows': "(self, E, Eb, re, batch, k: 'int' = 1)",
    'score_windows_plda': "(self, E, batch, k: 'int' = 1)",
    'score_windows_snorm': "(self, E, batch, k: 'int' = 1)",
    'segmentation': '(self)',
    'speaker_table': '(self, batch)',
    'speech_ranges': "(self, samples: 'np.ndarray', step_s: 'float' = 1.0)",
    'train_plda': "(self, samples_or_paths, references, uris=None, out_dir=None, D0: 'int' = 128, lda_dim: 'int' = 128, n_iters: 'int' = 10, step_s: 'float' = 1.0, speaker_key=None, logp=None)",
    'tune_diarization': '(self, samples_or_paths, references, thresholds, uris=None, **kw)',
    'tune_verification': "(self, audio_paths, speaker_ids, candidates, score_range=None, p_target: 'float' = 0.01, c_miss: 'float' = 1.0, c_fa: 'float' = 1.0, max_refine: 'int' = 8) -> 'Dict[str, Any]'",
    'verify_speaker': "(self, audio_path: 'Path', speaker_profile: 'Dict[str, Any]', threshold: 'float' = 0.354) -> 'Dict[str, Any]'",
}
# the rule settings the constructor used to assign: attributes of every instance then, properties that read and write the rule now
SETTINGS = {"cohort_path": None, "cohort_threshold": None, "cohort_topk": 300, "score_plda_paths": None, "score_plda_dim": 128,
            "score_plda_threshold": 0.0, "score_plda_count": True}
RULE_VARIABLES = ("SDK_COHORT", "SDK_COHORT_TOPK", "SDK_COHORT_THRESHOLD", "SDK_NO_TORCH", "SDK_SCORE_PLDA_TRANSFORM", "SDK_SCORE_PLDA",
                  "SDK_SCORE_PLDA_DIM", "SDK_SCORE_PLDA_THRESHOLD", "SDK_SCORE_PLDA_COUNT")


def plain_backend(monkeypatch):
    for v in RULE_VARIABLES:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("SDK_ECAPA_WEIGHTS", "unused.npz")             # only silences the synthetic-weights notice; nothing is loaded here
    return BK.Backend()


# ---- surface --------------------------------------------------------------------------------------------------------------------------
def test_backend_keeps_every_public_attribute_and_signature(monkeypatch):
    got = {}
    for name in (n for n in dir(BK.Backend) if not n.startswith("_") or n == "_plda_rows"):
        attr = inspect.getattr_static(BK.Backend, name)
        got[name] = "property" if isinstance(attr, property) else str(inspect.signature(getattr(BK.Backend, name)))
    assert {n: got.get(n) for n in PUBLIC} == PUBLIC
    assert sorted(set(got) - set(PUBLIC)) == sorted(SETTINGS)         # the class gained the settings' properties and no other public name
    be = plain_backend(monkeypatch)
    assert {n: getattr(be, n) for n in SETTINGS} == SETTINGS and be.rule.kind == "cosine" and be.plda_scoring is False
    assert be.cohort() is None and be.score_plda() is None and be._engine is None
    be.cohort_threshold, be.score_plda_threshold = 1.5, -2.0          # tests and tuning code assign the two thresholds
    assert (be.rule.cohort_threshold, be.rule.score_plda_threshold) == (1.5, -2.0)
    for name in ("aggregate_matches", "aggregate_matches_snorm", "plda_classes"):
        assert callable(getattr(BK, name)), name
    for name in ("_snorm_enqueue", "_plda_enqueue", "_aggregate_plda"):
        assert not hasattr(BK.Backend, name), name


def test_each_configuration_gives_its_rule_and_reads_no_file(monkeypatch):
    plain_backend(monkeypatch)
    monkeypatch.setenv("SDK_COHORT", "cohort.npy")
    monkeypatch.setenv("SDK_COHORT_THRESHOLD", "-1.25")
    monkeypatch.setenv("SDK_COHORT_TOPK", "40")
    be = BK.Backend()
    assert (be.rule.kind, be.rule.verify_keys) == ("snorm", ("norm_score",)) and isinstance(be.rule, RULES.Snorm)
    assert (be.cohort_path, be.cohort_threshold, be.cohort_topk, be.plda_scoring, be._engine) == ("cohort.npy", -1.25, 40, False, None)
    with pytest.raises(ValueError, match="AS-norm trials are not built"):
        be.rule.refuse_trials()                                       # score_verification's first step
    for v in ("SDK_COHORT", "SDK_COHORT_THRESHOLD"):
        monkeypatch.delenv(v)
    monkeypatch.setenv("SDK_SCORE_PLDA_TRANSFORM", "t.npz")
    monkeypatch.setenv("SDK_SCORE_PLDA", "p.npz")
    monkeypatch.setenv("SDK_SCORE_PLDA_DIM", "64")
    be = BK.Backend()
    assert (be.rule.kind, be.rule.verify_keys) == ("plda", ("llr",)) and isinstance(be.rule, RULES.Plda)
    assert (be.score_plda_paths, be.score_plda_dim, be.score_plda_threshold, be.score_plda_count) == (("t.npz", "p.npz"), 64, 0.0, True)
    assert be.plda_scoring is True and be.cohort_topk == 40 and be.cohort() is None and be._score_plda is None and be._engine is None


def test_importing_backend_and_rules_leaves_torch_out():
    code = (f"import importlib, sys; importlib.import_module('{PKG}.backend'); importlib.import_module('{PKG}.rules'); "
            "sys.exit(1 if 'torch' in sys.modules else 0)")
    assert subprocess.run([sys.executable, "-c", code], cwd=str(ROOT)).returncode == 0


# ---- aggregation ----------------------------------------------------------------------------------------------------------------------
def nan_as_text(rows):
    """A NaN is not equal to itself: the record holds the string "nan" for it, and so do the rows compared with it."""
    return [{k: "nan" if isinstance(v, float) and v != v else v for k, v in r.items()} for r in rows]


@pytest.fixture(scope="module")
def recorded():
    rec = json.loads((GOLDEN / "aggregate_rows.json").read_text())
    for lists in rec["rows"].values():
        for rows in lists:
            for r in rows:
                r["segment"] = tuple(r["segment"])
    case = rec["case"]
    case["idx"] = np.asarray(case["idx"], np.int32)
    case["cos"] = np.asarray([float(s) for s in case["cos"]], np.float32)          # float("nan") reads the record's "nan"
    case["spans"] = [tuple(s) for s in case["spans"]]
    return rec


def test_the_recorded_case_holds_every_edge(recorded):
    case, rows = recorded["case"], recorded["rows"]
    idx, cos = case["idx"], case["cos"]
    assert len(idx) == 40 and len(case["speaker_ids"]) == 7 and len(set(case["speaker_ids"])) == 4
    assert (idx == -1).any() and np.isnan(cos).any() and (cos == np.float32(case["thresholds"]["cosine"][0])).any()
    by = {r["speaker_id"]: r for r in rows["snorm"][0]}
    assert by["bob"]["norm_score"] == by["cy"]["norm_score"] and by["bob"]["similarity"] == by["cy"]["similarity"]      # equal means: by id
    ann = [int(p) for p, s in zip(idx, cos) if p in (0, 2) and s >= 0.5]
    assert ann.count(0) == ann.count(2) > 0 and ann[0] == 2 and by["ann"]["embedding_id"] == "e0"                      # equal wins: the first row
    assert rows["snorm"][1] == rows["plda"][1] == [] and [r["speaker_id"] for r in rows["cosine"][1]] == ["dee"]       # `s < threshold`: a NaN votes


@pytest.mark.parametrize("which", [0, 1])
def test_the_three_aggregations_answer_as_recorded(recorded, which):
    case, rows = recorded["case"], recorded["rows"]
    idx, cos, spans = case["idx"], case["cos"], case["spans"]

    class batch:
        speaker_ids, embedding_ids = case["speaker_ids"], case["embedding_ids"]
    thr = {k: v[which] for k, v in case["thresholds"].items()}
    assert nan_as_text(BK.aggregate_matches(idx, cos, spans, batch, thr["cosine"])) == rows["cosine"][which]
    assert nan_as_text(BK.aggregate_matches_snorm(idx, cos * np.float32(4), cos, spans, batch, thr["snorm"])) == rows["snorm"][which]
    group, speakers, first, counts = PS.group_speakers(batch.speaker_ids)
    sidx = np.where(idx >= 0, group[np.maximum(idx, 0)], -1).astype(np.int32)
    got = PS.aggregate_matches_plda(sidx, cos.astype(np.float64) * 8 - 4, spans, speakers, [batch.embedding_ids[int(p)] for p in first], counts, thr["plda"])
    assert nan_as_text(got) == rows["plda"][which]
    if which == 0:
        assert [list(r) for r in rows["cosine"][0]] == [["speaker_id", "similarity", "confidence", "embedding_id", "segment", "n_segments"]] * 4
        assert [list(r) for r in BK.aggregate_matches(idx, cos, spans, batch, thr["cosine"])] == [list(r) for r in rows["cosine"][0]]     # key order
        assert list(got[0]) == list(rows["plda"][0][0])


def test_cached_hits_on_the_same_engine_and_key_only():
    class Batch:
        pass
    batch, eng, other, made = Batch(), object(), object(), []

    def make():
        made.append(len(made))
        return made[-1]
    assert RULES.cached(batch, "_slot", eng, ("d", 3), make) == 0 and RULES.cached(batch, "_slot", eng, ("d", 3), make) == 0
    assert batch._slot == (eng, ("d", 3), 0)
    assert RULES.cached(batch, "_slot", eng, ("d", 4), make) == 1 and RULES.cached(batch, "_slot", other, ("d", 4), make) == 2
    assert RULES.cached(batch, "_dev", eng, None, make) == 3 and RULES.cached(batch, "_dev", eng, None, make) == 3 and made == [0, 1, 2, 3]


# ---- nothing waits --------------------------------------------------------------------------------------------------------------------
class FakeTensor:
    def __init__(self, log, tag, n):
        self.log, self.tag, self.n = log, tag, n

    def cpu(self):
        self.log.append(("cpu",) + self.tag)
        return self

    def numpy(self):
        return np.full((self.n, 1), self.tag[0], np.float64)


class StubRule:
    verify_keys = ()

    def __init__(self, kind, log):
        self.kind, self.log, self.columns = kind, log, 3 if kind == "snorm" else 2

    def enqueue(self, be, emb, batch, k=1):
        self.log.append(("enqueue", emb))
        return tuple(FakeTensor(self.log, (emb, c), 2 + emb) for c in range(self.columns))

    def rows(self, be, cols, spans, batch, threshold):
        assert len(cols) == self.columns and all(c.shape == (len(spans),) for c in cols)
        return [{"recording": int(cols[0][0]), "windows": len(spans), "threshold": threshold}]


@pytest.mark.parametrize("kind", ["cosine", "snorm", "plda"])
def test_identify_many_enqueues_every_recording_before_the_first_download(monkeypatch, kind):
    be, log = plain_backend(monkeypatch), []
    be.rule = StubRule(kind, log)
    be._load_candidates = lambda candidates: ["one enrolled embedding"]
    be._windows = lambda path, segments: (log.append(("windows", path)) or path, "starts", 32000, [(float(w), w + 2.0) for w in range(2 + path)])
    be.embed_tables = lambda samples, tables: log.append(("embed",)) or {32000: samples}          # the "embeddings": the recording's number
    out = be.identify_many([0, 1, 2], candidates=[], threshold=0.25)
    assert out == [[{"recording": r, "windows": 2 + r, "threshold": 0.25}] for r in range(3)]
    first_cpu = next(i for i, e in enumerate(log) if e[0] == "cpu")
    assert [e for e in log[:first_cpu] if e[0] == "enqueue"] == [("enqueue", r) for r in range(3)] and first_cpu == 9
    assert log[:first_cpu] == [e for r in range(3) for e in (("windows", r), ("embed",), ("enqueue", r))]
    n = be.rule.columns
    assert log[first_cpu:] == [("cpu", r, c) for r in range(3) for c in range(n)]         # then one collection pass, in order
    assert be._engine is None
    log.clear()
    assert be.identify_speaker(1, candidates=[]) == [{"recording": 1, "windows": 3, "threshold": 0.354}]
    assert log == [("windows", 1), ("embed",), ("enqueue", 1)] + [("cpu", 1, c) for c in range(n)]
    be._load_candidates = lambda candidates: []
    assert be.identify_many([0, 1], []) == [[], []] and be.identify_speaker(0, []) == []


# ---- refusal order --------------------------------------------------------------------------------------------------------------------
def test_the_refusals_come_in_their_order(monkeypatch):
    env = {"SDK_COHORT": "cohort.npy", "SDK_COHORT_TOPK": "0", "SDK_NO_TORCH": "1", "SDK_SCORE_PLDA_TRANSFORM": "t.npz", "SDK_SCORE_PLDA_DIM": "96",
           "SDK_SCORE_PLDA_THRESHOLD": "low", "SDK_SCORE_PLDA_COUNT": "2"}

    def refusal():
        with pytest.raises(ValueError) as exc:
            RULES.rule_from_env(env)
        return str(exc.value)

    assert refusal().startswith("SDK_COHORT (the cohort file) and SDK_COHORT_THRESHOLD") and "SDK_COHORT_THRESHOLD is not set" in refusal()
    plain_backend(monkeypatch)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with pytest.raises(ValueError, match="SDK_COHORT .*SDK_COHORT_THRESHOLD is not set"):              # the Backend's constructor says the same
        BK.Backend()
    env["SDK_COHORT_THRESHOLD"] = "high"
    assert refusal().startswith("SDK_COHORT_THRESHOLD='high'")
    env["SDK_COHORT_THRESHOLD"] = "nan"
    assert refusal().startswith("SDK_COHORT_THRESHOLD is NaN")
    env["SDK_COHORT_THRESHOLD"] = "2.5"
    assert refusal().startswith("SDK_COHORT_TOPK=0")
    env["SDK_COHORT_TOPK"] = "300"
    assert refusal().startswith("SDK_COHORT with SDK_NO_TORCH=1")
    del env["SDK_NO_TORCH"]
    assert refusal().startswith("SDK_SCORE_PLDA_TRANSFORM and SDK_SCORE_PLDA name the two files") and "(SDK_SCORE_PLDA is not set)" in refusal()
    monkeypatch.setenv("SDK_COHORT_THRESHOLD", "2.5")
    monkeypatch.setenv("SDK_COHORT_TOPK", "300")
    monkeypatch.delenv("SDK_NO_TORCH")
    with pytest.raises(ValueError, match="SDK_SCORE_PLDA_TRANSFORM and SDK_SCORE_PLDA name the two files"):
        BK.Backend()
    env["SDK_SCORE_PLDA"] = "p.npz"
    assert refusal().startswith("SDK_SCORE_PLDA* together with SDK_COHORT")
    del env["SDK_COHORT"], env["SDK_COHORT_THRESHOLD"]
    env["SDK_NO_TORCH"] = "1"
    assert refusal().startswith("SDK_SCORE_PLDA* with SDK_NO_TORCH=1")
    del env["SDK_NO_TORCH"]
    assert refusal().startswith("SDK_SCORE_PLDA_DIM='96'")
    env["SDK_SCORE_PLDA_DIM"] = "64"
    assert refusal().startswith("SDK_SCORE_PLDA_THRESHOLD='low'")
    env["SDK_SCORE_PLDA_THRESHOLD"] = "nan"
    assert refusal().startswith("SDK_SCORE_PLDA_THRESHOLD is NaN")
    env["SDK_SCORE_PLDA_THRESHOLD"] = "-1"
    assert refusal().startswith("SDK_SCORE_PLDA_COUNT='2'")
    env["SDK_SCORE_PLDA_COUNT"] = "0"
    rule = RULES.rule_from_env(env)
    assert (rule.kind, rule.score_plda_paths, rule.score_plda_dim, rule.score_plda_threshold, rule.score_plda_count) == ("plda", ("t.npz", "p.npz"), 64, -1.0, False)
    assert RULES.rule_from_env({}).kind == "cosine" and RULES.rule_from_env({"SDK_COHORT": "c.npy", "SDK_COHORT_THRESHOLD": "0"}).kind == "snorm"
