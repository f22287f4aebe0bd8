"""CPU checks of the diarization's module layout: diarize.py states the rule and holds the Diarizer; the host layer (diarize_host.py), the
device wrappers (diarize_ops.py) and the linking (diarize_link.py) are modules of their own, re-exported by diarize.py name by name, and
diarize_ops.py is a leaf that cluster.py, score.py and stream.py can import without meeting diarize.py."""
from __future__ import annotations

import importlib
import inspect
import os
import subprocess
import sys

import pytest

PKG = "speaker-diarization-toolkit_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every name diarize.py defined while it was one module (what tests, tools, backend.py and stream.py take from it), by its home today
HOMES = {
    "diarize_host": """MIN_CLEAN_COLUMNS MIN_VALID_COLUMNS TRAIN_CLEAN_DEN MAX_LINKAGE_ROWS DEFAULT_BATCH N_LOCAL MAX_ASSIGN_DIM MAX_PACK_SAMPLES
        DEFAULT_PACK_SAMPLES DEFAULT_PACK_LINKAGE_BYTES _MASK _COUNT DiarizationResult Pack pack_recordings global_frames decode_host masks_host
        reconstruct_host _speaker_cap candidate_mask training_mask training_rows assign_rows _centroids64 constrained_chunk
        assign_constrained_host appearance_order turns_from_frames to_rttm _dot_in_order assign_grouped_host fold_grouped_host
        reconstruct_grouped_host first_seen_host renumber_host""".split(),
    "diarize_ops": """VBX_HOST_READS LINKAGE_HOST_READS _native _check_dim _check_rows _check_tensor GroupTables powerset_decode diarize_masks
        diarize_reconstruct diarize_centroids diarize_assign diarize_assign_grouped diarize_fold_grouped diarize_reconstruct_grouped
        diarize_first_seen diarize_renumber""".split(),
    "diarize_link": "SpeakerLinks link_speakers relabel_turns".split(),
    "diarize": ["Diarizer"],
}


@pytest.mark.parametrize("home", sorted(HOMES))
def test_every_name_is_reexported_from_its_home(home):
    dz, mod = importlib.import_module(f"{PKG}.diarize"), importlib.import_module(f"{PKG}.{home}")
    for name in HOMES[home]:
        assert getattr(dz, name) is getattr(mod, name), name
        if inspect.isclass(getattr(mod, name)) or inspect.isfunction(getattr(mod, name)):
            assert getattr(mod, name).__module__ == mod.__name__, name       # defined there, not passed through


def test_ops_is_a_leaf():
    """diarize_ops imports in a fresh process without diarize, cluster, score or stream - and without torch, which _native brings at the
    first call."""
    code = (f"import importlib, sys\n"
            f"importlib.import_module('{PKG}.diarize_ops')\n"
            f"bad = [m for m in ('diarize', 'cluster', 'score', 'stream') if '{PKG}.' + m in sys.modules] + [m for m in ('torch',) if m in sys.modules]\n"
            f"assert not bad, bad\n")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_private_stages_take_records():
    """No private method of Diarizer takes more than four parameters besides self: the stages take the pack, the clusters and the options
    as records.  _check_options alone keeps its five, which tests/test_speaker_bounds_cpu.py calls by position."""
    dz = importlib.import_module(f"{PKG}.diarize")
    long = {name: len(inspect.signature(f).parameters) - 1 for name, f in vars(dz.Diarizer).items()
            if inspect.isfunction(f) and name.startswith("_") and not name.startswith("__") and len(inspect.signature(f).parameters) - 1 > 4}
    assert long == {"_check_options": 5}
