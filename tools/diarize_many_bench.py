#!/usr/bin/env python3
"""Diarization of many recordings: Diarizer.run_many on a generated folder (256 x 3 min and 32 x 30 min at a 1-s step; the generator is
tools/diarize_bench.py's amplitude-modulated noise, one seed per recording) beside a loop of Diarizer.run(constrained=True) - the
single-recording path, unchanged - over the same recordings in the same process.  Wall clock around the whole call (each ends with its own
downloads, so the device is idle when it returns), best of three after a warm-up.  One JSON line: per configuration the total time,
recordings/s, the real-time factor, the per-stage split of run_many (a separate traced pass: every stage ended by a device
synchronisation) and the number of waits for the device per pack.  Record the line in profiles/r13_diarize_many_bench.json.  Synthetic
weights: the class table is the model's own (noise-like) output, which exercises every stage at full size."""
from __future__ import annotations

import argparse
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PKG = "speaker-diarization-toolkit_amd"


def recording(seed: int, n: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n, dtype=np.float32) * np.float32(0.1) * (1 + np.sin(2 * np.pi * 0.3 * np.arange(n, dtype=np.float32) / 16000))
    return np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="256x180,32x1800", help="comma-separated RxSECONDS")
    ap.add_argument("--step", type=float, default=1.0)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    import torch
    ops = importlib.import_module(f"{PKG}.ops")
    seg = importlib.import_module(f"{PKG}.segmentation")
    rn = importlib.import_module(f"{PKG}.resnet")
    dz = importlib.import_module(f"{PKG}.diarize")
    eng = ops.get_engine(0)
    diar = dz.Diarizer(eng, seg.Segmentation(eng, seg.synthetic_weights(0)), rn.ResNet34(eng, rn.synthetic_weights(0)))
    kw = dict(step_s=a.step, threshold=a.threshold, constrained=True)
    out = {"tool": "diarize_many_bench", "step_s": a.step, "threshold": a.threshold, "configs": []}
    for cfg in a.configs.split(","):
        R, secs = (int(v) for v in cfg.split("x"))
        recs = [recording(r, secs * 16000) for r in range(R)]
        diar.run_many(recs[:2], **kw)                                     # warm-up: code objects, scratch buffers
        diar.run(recs[0], **kw)
        t_many, t_loop = [], []
        for _ in range(a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            many = diar.run_many(recs, **kw)
            t_many.append(time.perf_counter() - t0)
        syncs = diar.last_sync
        for _ in range(a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop = [diar.run(x, **kw) for x in recs]
            t_loop.append(time.perf_counter() - t0)
        diar.trace, diar.last_stage_s = True, []
        diar.run_many(recs, **kw)
        diar.trace = False
        stages = {}
        for p in diar.last_stage_s:
            for k, v in p.items():
                stages[k] = stages.get(k, 0.0) + v
        same = all(np.array_equal(m.labels, l.labels) and np.array_equal(m.speakers, l.speakers) and m.turns == l.turns for m, l in zip(many, loop))
        audio = R * secs
        out["configs"].append({"recordings": R, "seconds_each": secs, "chunks": int(sum(len(m.starts) for m in many)), "packs": len(syncs),
                               "run_many_s": round(min(t_many), 4), "run_loop_s": round(min(t_loop), 4),
                               "run_many_recordings_per_s": round(R / min(t_many), 2), "run_loop_recordings_per_s": round(R / min(t_loop), 2),
                               "run_many_real_time_factor": round(min(t_many) / audio, 7), "run_loop_real_time_factor": round(min(t_loop) / audio, 7),
                               "speedup": round(min(t_loop) / min(t_many), 3), "run_many_stage_ms_traced": {k: round(v * 1e3, 2) for k, v in stages.items()},
                               "waits_for_the_device_per_pack": syncs[0], "results_equal_the_loop": bool(same),
                               "clusters": [int(np.min([m.n_speakers for m in many])), int(np.max([m.n_speakers for m in many]))]})
        del recs, many, loop
    print(json.dumps(out))


if __name__ == "__main__":
    main()
