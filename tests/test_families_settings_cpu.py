"""CPU checks of the family table (families.py) and the call-time settings readers (settings.py) behind the Backend: every row says what
the Backend answers for its SDK_MODEL, the shared .npz loader refuses a malformed file by the tensor's name, every reader follows a
variable changed on a live Backend, and the refusals that moved with them are raised in their words."""
from __future__ import annotations

import os

import numpy as np
import pytest
from conftest import sub

BK = sub("backend")
FAM = sub("families")
SET = sub("settings")
CONFIGS = {"ecapa": sub("weights").DEFAULT_CONFIG, "xvector": sub("xvector").DEFAULT_XVECTOR, "resnet34": sub("resnet").DEFAULT_RESNET}
VARIABLES = ("SDK_MODEL", "SDK_DIARIZE_MODEL", "SDK_PRECISION", "SDK_NO_TORCH", "SDK_DEVICE", "LOCAL_RANK", "SDK_MAX_BATCH", "SDK_SEGMENTATION_BATCH",
             "SDK_ECAPA_WEIGHTS", "SDK_XVECTOR_WEIGHTS", "SDK_RESNET_WEIGHTS", "SDK_SEGMENTATION_WEIGHTS", "SDK_ECAPA_LAYOUT", "SDK_ECAPA_PREFIX",
             "SDK_CACHE_BUILD_TIMEOUT_S", "SDK_PLDA_TRANSFORM", "SDK_PLDA", "SDK_PLDA_DIM", "SDK_COHORT", "SDK_COHORT_THRESHOLD",
             "SDK_SCORE_PLDA_TRANSFORM", "SDK_SCORE_PLDA")


@pytest.fixture
def backend_for(monkeypatch):
    for v in VARIABLES:
        monkeypatch.delenv(v, raising=False)

    def make(model: str = "ecapa"):
        monkeypatch.setenv("SDK_MODEL", model)
        return BK.Backend()
    return make


def test_the_table_has_the_three_families():
    assert list(FAM.FAMILIES) == ["ecapa", "xvector", "resnet34"] and all(f.name == k for k, f in FAM.FAMILIES.items())
    with pytest.raises(Exception):                                  # frozen: a row is not a place to keep state
        FAM.FAMILIES["ecapa"].cached = False


@pytest.mark.parametrize("model", ["ecapa", "xvector", "resnet34"])
def test_a_row_says_what_the_backend_answers(backend_for, monkeypatch, capsys, model):
    monkeypatch.setenv("SDK_BIAS_CORRECTION", "1")
    fam, cfg = FAM.FAMILIES[model], CONFIGS[model]
    tag = {"ecapa": lambda: f"ecapa{cfg.channels}", "xvector": lambda: f"xvector{cfg.channels[0]}", "resnet34": lambda: "resnet34"}[model]()
    be = backend_for(model)
    assert f"{fam.weights_env} not set - using seeded synthetic {fam.label} weights" in capsys.readouterr().err
    assert fam.config is cfg and fam.embed_dim == cfg.embed_dim == be.embedding_dim and fam.version_tag == tag
    be._digest = "0" * 12                                           # the digest is the weights' business: nothing is generated or hashed here
    assert be.model_version == f"{be.name}-{tag}-{'0' * 12}" and be._weights is None
    assert (be._cache_key() is not None) == fam.cached == (model == "ecapa")
    assert be.numerics() == {"precision": 0, "bias_correction": fam.bias_correction} and fam.bias_correction == (model != "resnet34")
    assert fam.precisions == ((0, 2) if model == "resnet34" else (0, 1, 2)) and fam.lite == (model != "resnet34")
    assert (fam.extractor_name is None) == (model == "ecapa") and be._engine is None


@pytest.mark.parametrize("model,tensor", [("xvector", None), ("resnet34", "seg_1.weight")])
def test_the_shared_loader_checks_shapes_by_name(backend_for, monkeypatch, tmp_path, model, tensor):
    fam = FAM.FAMILIES[model]
    w = fam.synthetic()
    tensor = tensor or sorted(k for k, v in w.items() if v.ndim >= 2)[0]
    np.savez(tmp_path / "good.npz", **{k: v.astype(np.float64) for k, v in w.items()})
    got = FAM.load_npz_weights(tmp_path / "good.npz", fam.check)
    assert sorted(got) == sorted(w) and all(got[k].dtype == np.float32 and got[k].flags.c_contiguous and np.array_equal(got[k], w[k]) for k in w)
    bad = dict(w)
    bad[tensor] = bad[tensor][:, :-1]
    np.savez(tmp_path / "bad.npz", **bad)
    with pytest.raises(ValueError, match=tensor.replace(".", r"\.")):
        FAM.load_npz_weights(tmp_path / "bad.npz", fam.check)
    monkeypatch.setenv(fam.weights_env, str(tmp_path / "bad.npz"))
    with pytest.raises(ValueError, match=tensor.replace(".", r"\.")):
        fam.host_weights()                                          # the one loader behind Backend._host_weights and Backend.diarizer
    be = backend_for(model)
    with pytest.raises(ValueError, match=tensor.replace(".", r"\.")):
        be.model_version


def test_every_reader_follows_the_environment_of_a_live_backend(backend_for, monkeypatch):
    be = backend_for()
    assert (SET.device(), SET.precision(), SET.precision_text(), SET.max_batch(), SET.segmentation_batch()) == (0, 0, None, 2048, 256)
    assert (SET.lite(), be.lite, SET.bias_correction()) == (False, False, os.environ.get("SDK_BIAS_CORRECTION", "1") != "0")
    assert (SET.weights_path("SDK_ECAPA_WEIGHTS"), SET.ecapa_layout(), SET.ecapa_prefix(), SET.cache_build_timeout_s()) == (None, "native", "", 300.0)
    assert SET.diarizer_plda() is None
    monkeypatch.setenv("LOCAL_RANK", "3")
    assert SET.device() == 3
    monkeypatch.setenv("SDK_DEVICE", "5")
    assert SET.device() == 5
    monkeypatch.setenv("SDK_PRECISION", " 2 ")
    assert (SET.precision(), SET.precision_text(), be.numerics()["precision"]) == (2, " 2 ", 2)
    monkeypatch.setenv("SDK_MAX_BATCH", "7")
    monkeypatch.setenv("SDK_SEGMENTATION_BATCH", "0")
    assert (SET.max_batch(), SET.segmentation_batch()) == (7, 1)
    monkeypatch.setenv("SDK_MAX_BATCH", "-4")
    assert SET.max_batch() == 1
    monkeypatch.setenv("SDK_NO_TORCH", "1")
    assert SET.lite() is True and be.lite is True
    monkeypatch.setenv("SDK_NO_TORCH", "true")
    assert SET.lite() is False and be.lite is False
    monkeypatch.setenv("SDK_BIAS_CORRECTION", "1")
    assert SET.bias_correction() is True and be.numerics() == {"precision": 2, "bias_correction": True}
    monkeypatch.setenv("SDK_BIAS_CORRECTION", "0")
    assert SET.bias_correction() is False and be.numerics() == {"precision": 2, "bias_correction": False}
    monkeypatch.setenv("SDK_ECAPA_WEIGHTS", "w.npz")
    monkeypatch.setenv("SDK_ECAPA_LAYOUT", "public")
    monkeypatch.setenv("SDK_ECAPA_PREFIX", "model.")
    monkeypatch.setenv("SDK_CACHE_BUILD_TIMEOUT_S", "1.5")
    assert (SET.weights_path("SDK_ECAPA_WEIGHTS"), SET.ecapa_layout(), SET.ecapa_prefix(), SET.cache_build_timeout_s()) == ("w.npz", "public", "model.", 1.5)
    monkeypatch.setenv("SDK_PLDA_TRANSFORM", "t.npz")
    with pytest.raises(ValueError, match="SDK_PLDA_TRANSFORM and SDK_PLDA name the two files of one PLDA model: set both or neither"):
        SET.diarizer_plda()
    monkeypatch.setenv("SDK_PLDA", "p.npz")
    assert SET.diarizer_plda() == ("t.npz", "p.npz", 128)
    monkeypatch.setenv("SDK_PLDA_DIM", "64")
    assert SET.diarizer_plda() == ("t.npz", "p.npz", 64)
    monkeypatch.setenv("SDK_PLDA_DIM", "96")
    with pytest.raises(ValueError, match=r"SDK_PLDA_DIM='96': the PLDA dimensions kept, 64 or 128"):
        SET.diarizer_plda()
    monkeypatch.delenv("SDK_PLDA_TRANSFORM")
    with pytest.raises(ValueError, match="SDK_PLDA_TRANSFORM and SDK_PLDA name the two files"):
        SET.diarizer_plda()
    assert be._engine is None


def test_the_refusals_that_moved_keep_their_words(backend_for, monkeypatch):
    be = backend_for("resnet34")
    monkeypatch.setenv("SDK_NO_TORCH", "1")
    monkeypatch.setenv("SDK_PRECISION", "1")                        # the family is refused before the precision is looked at
    with pytest.raises(ValueError, match=r"SDK_NO_TORCH=1 with SDK_MODEL=resnet34: the torch-free host path does not serve the ResNet34 family; unset SDK_NO_TORCH"):
        be.engine()
    for name, what in (("segmentation", "speech_ranges"), ("diarizer", "diarize")):
        with pytest.raises(ValueError, match=f"{what} needs the torch engine: not available with SDK_NO_TORCH=1"):
            getattr(be, name)()
    monkeypatch.delenv("SDK_NO_TORCH")
    with pytest.raises(ValueError, match=r"SDK_PRECISION=1 \(the precise mode\) is not built for SDK_MODEL=resnet34: use SDK_PRECISION=0 or 2"):
        be.engine()
    with pytest.raises(ValueError, match=r"SDK_PRECISION=1 \(the precise mode\) is not built for the segmentation model: use SDK_PRECISION=0 or 2"):
        be.segmentation()
    assert be._engine is None and be._extractor is None
    for model in ("ecapa", "xvector"):
        be = backend_for(model)
        monkeypatch.setenv("SDK_NO_TORCH", "1")
        with pytest.raises(ValueError, match=r"SDK_NO_TORCH=1 serves the single-plane contracts \(SDK_PRECISION=0 or 2\); SDK_PRECISION=1 needs the torch engine"):
            be.engine()
        monkeypatch.delenv("SDK_NO_TORCH")
    monkeypatch.setenv("SDK_DIARIZE_MODEL", "ecapa")
    monkeypatch.setenv("SDK_PRECISION", " 1")
    with pytest.raises(ValueError, match=r"SDK_DIARIZE_MODEL=ecapa requires SDK_PRECISION 0 \(bf16\) or 2 \(fp16\).*got SDK_PRECISION=' 1'"):
        backend_for("ecapa")
    monkeypatch.setenv("SDK_PRECISION", " 2 ")                      # the constructor strips the value before it compares it
    assert backend_for("ecapa").diarize_model == "ecapa"
    monkeypatch.setenv("SDK_MODEL", "wav2vec")
    with pytest.raises(ValueError, match=r"SDK_MODEL='wav2vec': expected 'ecapa', 'xvector' or 'resnet34'"):
        BK.Backend()
