#!/usr/bin/env python3
"""Fusing several diarizations on the device (fuse.py, csrc/fuse.hip) on one MI355X -> one JSON line.

For every --configs entry RxSECONDS (default 256 x 3 min and one hour) and H = 3 and 8: tools/der_bench.py's generated frame tables
(4 speakers, rows of every kind) as the first hypothesis and H - 1 noisy relabelled copies (an eighth of the frames renamed, the speaker
numbers permuted); fuse.fuse_results - host preparation, the one upload, the launches, the one download and the cutting of turns - beside
the same with fuse.fuse_host in the device's place (wall clock, minimum and median of --iters windows after a warm-up), every launch alone
(a window of WINDOW back-to-back calls between two events, divided by WINDOW), sdk_score_cooccur over the same frames as the bandwidth
yardstick, and whether every table agrees with the host's.  No time is a pass condition.  Record the line in profiles/r38_fuse_bench.json.
    python tools/fuse_bench.py [--configs 256x180,1x3600] [--hyps 3,8] [--iters 3]"""
from __future__ import annotations

import argparse
import importlib
import json
import statistics
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
PKG = "speaker-diarization-toolkit_amd"
WINDOW = 20

import der_bench as DB  # noqa: E402


def noisy_copy(sp: np.ndarray, seed: int, K: int = 4) -> np.ndarray:
    rng = np.random.default_rng(seed)
    out = sp.copy()
    at = rng.choice(len(sp), size=len(sp) // 8, replace=False)
    out[at, 0] = rng.integers(-1, K, len(at))
    perm = rng.permutation(K)
    return np.where(out >= 0, perm[np.maximum(out, 0)], -1).astype(np.int32)


def device_ms(fn, iters: int):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    ts = []
    for _ in range(iters):
        e0.record()
        for _ in range(WINDOW):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / WINDOW)
    return {"min": round(min(ts), 4), "median": round(statistics.median(ts), 4)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="256x180,1x3600")
    ap.add_argument("--hyps", default="3,8")
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    import torch
    ops, dz, sc, fu = (importlib.import_module(f"{PKG}.{m}") for m in ("ops", "diarize", "score", "fuse"))
    eng = ops.get_engine(0)
    out = {"tool": "fuse_bench", "iters": a.iters, "window": WINDOW, "runs": []}
    for cfg in a.configs.split(","):
        R, secs = (int(v) for v in cfg.split("x"))
        n = secs * 16000
        G = dz.global_frames(n)
        base = [DB.hypothesis(1000 + r, G) for r in range(R)]
        for H in (int(h) for h in a.hyps.split(",")):
            hyps = [[SimpleNamespace(speakers=sp if h == 0 else noisy_copy(sp, 7919 * h + r), n_speakers=4) for h in range(H)] for r, sp in enumerate(base)]

            def on_host():
                pk = fu.prepare("fuse", hyps)
                return fu.assemble(pk, hyps, fu.fuse_host(fu.masks_of(pk), pk.tab.frame_off, pk.tab.K))
            fu.fuse_results(eng, hyps)                                    # warm-up: code objects
            dev, t_dev = DB.windows(lambda: fu.fuse_results(eng, hyps), a.iters)
            host, t_host = DB.windows(on_host, 1)
            same = all(np.array_equal(x.speakers, y.speakers) and x.turns == y.turns and x.n_speakers == y.n_speakers
                       and {k: (v.tolist() if k == "dis" else v) for k, v in x.fusion.items()} == {k: (v.tolist() if k == "dis" else v) for k, v in y.fusion.items()}
                       for x, y in zip(dev, host))
            # every launch alone, on tables left on the device
            pk = fu.prepare("fuse", hyps)
            tab = pk.tab.to(eng)
            sp_d = torch.from_numpy(np.concatenate([h[0].speakers for h in hyps])).to(eng.device)
            mask = torch.from_numpy(fu.masks_of(pk).view(np.int64)).to(eng.device)
            row = torch.empty((tab.G,), dtype=torch.int64, device=eng.device)
            co, tally = fu.fuse_cooccur(eng, mask, tab)
            _, correct = fu.pair_map(eng, co, tab)
            dis, order, weight, label_of, n_labels, overflow = fu.fuse_labels(eng, co, tally, correct, tab)
            launches = {"sdk_fuse_masks_one_hypothesis": device_ms(lambda: fu.fuse_masks(eng, sp_d, tab, 0, out=row), a.iters),
                        "sdk_fuse_cooccur": device_ms(lambda: fu.fuse_cooccur(eng, mask, tab), a.iters),
                        "sdk_score_map_on_the_pairs": device_ms(lambda: fu.pair_map(eng, co, tab), a.iters),
                        "sdk_fuse_labels": device_ms(lambda: fu.fuse_labels(eng, co, tally, correct, tab), a.iters),
                        "sdk_fuse_vote": device_ms(lambda: fu.fuse_vote(eng, mask, label_of, weight, overflow, tab, 2), a.iters)}
            # the yardstick: sdk_score_cooccur over the same frames (der_bench's references, no collar)
            gt = dz.GroupTables(eng, np.zeros(R + 1, np.int64), np.arange(R + 1, dtype=np.int64) * G, [n] * R).set_clusters(np.arange(R + 1) * 4)
            ref = sc.rasterise_references(eng, gt, [DB.reference(r, secs) for r in range(R)], 0.0, False)
            launches["sdk_score_cooccur_and_map_yardstick"] = device_ms(lambda: sc.score_tables(eng, sp_d, gt, ref), a.iters)
            out["runs"].append({"recordings": R, "seconds_each": secs, "frames": R * G, "hypotheses": H, "pairs": tab.P, "fuse_results": t_dev,
                                "fuse_host_path": t_host, "speedup_min": round(t_host["min_s"] / t_dev["min_s"], 2), "launch_ms": launches,
                                "tables_equal_the_host": bool(same), "unanimous_share": round(sum(x.fusion["unanimous"] for x in dev) / max(R * G, 1), 4),
                                "labels_max": max(x.n_speakers for x in dev)})
            del mask, sp_d, hyps
    print(json.dumps(out))


if __name__ == "__main__":
    main()
