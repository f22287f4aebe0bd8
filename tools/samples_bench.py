#!/usr/bin/env python3
"""Speaker samples on the device (samples.py, csrc/samples.hip) on one MI355X -> one JSON line.

For 256 x 3 min and for one hour of generated hypothesis tables (tools/words_bench.py's generator: 4 speakers, rows of every kind) on the
packed frame grid:
  runs             samples.runs - host preparation, the upload, sdk_samples_runs's nine launches and the two downloads - beside a loop of
                   samples.runs_host over the same recordings in the same process (wall clock, minimum and median of --iters windows after
                   a warm-up), and whether every row agrees
  device           the device time of sdk_samples_runs alone (a window of WINDOW back-to-back calls between two events, divided by WINDOW)
                   and, as a bandwidth yardstick, that of sdk_score_cooccur over the same frames (it reads 17 bytes per frame once;
                   sdk_samples_runs reads the 8 bytes of a frame once and then moves 4-byte words of its own: bytes_moved_runs counts them)
  score            sdk_samples_score at 10 speakers per recording, 8 clips a speaker and 1 - 8 windows a clip of generated unit rows
                   (d = 192) - samples.score with its upload and download, and the three launches alone - beside samples.score_host, and
                   the largest difference between the two
Record the line in profiles/r34_samples_bench.json.
    python tools/samples_bench.py [--iters 3]"""
from __future__ import annotations

import argparse
import importlib
import json
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
PKG = "speaker-diarization-toolkit_amd"
WINDOW = 20
CONFIGS = [("256x180s", 256, 180.0), ("1x3600s", 1, 3600.0)]
SPEAKERS, CLIPS, DIM = 10, 8, 192


def clips_of(seed: int, R: int):
    rng = np.random.default_rng(seed)
    S, M = R * SPEAKERS, R * SPEAKERS * CLIPS
    clip_spk = np.concatenate([r * SPEAKERS + rng.permutation(np.repeat(np.arange(SPEAKERS), CLIPS)) for r in range(R)])
    counts = rng.integers(1, 9, M)
    base = rng.standard_normal((S, DIM)).astype(np.float32)
    E = np.repeat(base[clip_spk], counts, axis=0) + rng.standard_normal((int(counts.sum()), DIM), dtype=np.float32) * np.float32(0.08)
    E /= np.linalg.norm(E, axis=1, keepdims=True)
    return E, np.concatenate([[0], np.cumsum(counts)]), clip_spk, np.arange(R + 1) * SPEAKERS


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    args = ap.parse_args()
    import torch
    from words_bench import hypothesis, timed
    ops, sm, sc, dz, ops_score = (importlib.import_module(f"{PKG}.{m}") for m in ("ops", "samples", "score", "diarize", "ops_score"))
    lib = importlib.import_module(f"{PKG}._lib")
    eng = ops.get_engine(0)
    gap, min_frames = sm.gap_frames(sm.DEFAULT_MAX_GAP_S), sm.min_frames_of(sm.DEFAULT_MIN_S)

    def device_ms(fn):
        fn()
        torch.cuda.synchronize()
        best = []
        for _ in range(max(args.iters, 3)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(WINDOW):
                fn()
            b.record()
            torch.cuda.synchronize()
            best.append(a.elapsed_time(b) / WINDOW)
        return round(min(best), 4)

    out = {"tool": "samples_bench", "device": lib.device_info(0)["name"], "iters": args.iters, "window": WINDOW, "gap_frames": gap, "min_frames": min_frames,
           "configs": {}}
    for name, R, secs in CONFIGS:
        G = dz.global_frames(int(secs * 16000))
        results = [SimpleNamespace(speakers=hypothesis(1000 + r, G), n_speakers=4) for r in range(R)]
        cfg = {"recordings": R, "frames": R * G}
        rows = sm.runs(eng, results)
        host = [sm.runs_host(res.speakers, 4, gap, min_frames) for res in results]
        cfg["runs"] = int(sum(len(h) for h in host))
        cfg["rows_agree"] = all(np.array_equal(a, b) for a, b in zip(rows, host))
        cfg["runs_device_path"] = timed(lambda: sm.runs(eng, results), args.iters)
        cfg["runs_host"] = timed(lambda: [sm.runs_host(res.speakers, 4, gap, min_frames) for res in results], args.iters)
        # the kernels alone, on resident tables
        tab = dz.GroupTables(eng, np.zeros(R + 1, np.int64), np.arange(R + 1, dtype=np.int64) * G, [270 * G + 226] * R)
        tab.set_clusters(np.arange(R + 1, dtype=np.int64) * 4)
        sp_d = torch.from_numpy(np.concatenate([res.speakers for res in results])).to(eng.device)
        cfg["device_runs_ms"] = device_ms(lambda: ops_score.samples_runs(eng, sp_d, tab.frame_off_d, tab.cent_off_d, 4, gap, min_frames))
        pref = sc.rasterise_references(eng, tab, [[(0.0, secs, "a")] for _ in range(R)])
        co_s, tally_s = torch.empty((R * 4,), dtype=torch.int32, device=eng.device), torch.empty((R, 5), dtype=torch.int64, device=eng.device)
        co_off_s = torch.arange(R + 1, dtype=torch.int64, device=eng.device) * 4
        cfg["device_score_cooccur_ms"] = device_ms(lambda: lib.check(eng.lib.sdk_score_cooccur(
            eng.ctx, pref.ref_mask.data_ptr(), pref.scored.data_ptr(), sp_d.data_ptr(), tab.frame_off_d.data_ptr(), pref.ref_off_d.data_ptr(),
            tab.cent_off_d.data_ptr(), co_off_s.data_ptr(), R, tab.G, pref.max_ref, 4, R * 4, co_s.data_ptr(), tally_s.data_ptr(), None), "sdk_score_cooccur"))
        groups = int(sum(int((np.diff(sm.frame_kinds(res.speakers, 4)[sm.frame_kinds(res.speakers, 4) != sm.SILENT]) != 0).sum()) + 1 for res in results))
        cfg["bytes_moved_runs"] = int(R * G * (8 + 4 + 4 + 4) + groups * (12 + 16 + 16) + cfg["runs"] * 20)        # an estimate: the groups split further at long pauses
        cfg["bytes_read_score_cooccur"] = int(17 * R * G)
        # the scores
        E, clip_off, clip_spk, spk_off = clips_of(3000 + R, R)
        E_d = torch.from_numpy(E).to(eng.device)
        got = sm.score(eng, E_d, clip_off, clip_spk, spk_off)
        want = sm.score_host(E, clip_off, clip_spk, spk_off)
        cfg["score"] = {"windows": int(len(E)), "clips": int(len(clip_spk)), "speakers": int(spk_off[-1]), "d": DIM,
                        "max_abs_difference": float(max(np.abs(got[0] - want[0]).max(), np.abs(got[1] - want[1]).max())),
                        "integers_agree": bool(np.array_equal(got[2], want[2])),
                        "device_path": timed(lambda: sm.score(eng, E_d, clip_off, clip_spk, spk_off), args.iters),
                        "host": timed(lambda: sm.score_host(E, clip_off, clip_spk, spk_off), args.iters)}
        up = torch.from_numpy(np.concatenate([clip_off, clip_spk, spk_off]).astype(np.int32)).to(eng.device)
        M = len(clip_spk)
        cfg["score"]["device_ms"] = device_ms(lambda: ops_score.samples_score(eng, E_d, up[:M + 1], up[M + 1:2 * M + 1], up[2 * M + 1:], int(spk_off[-1])))
        out["configs"][name] = cfg
    print(json.dumps(out))


if __name__ == "__main__":
    main()
