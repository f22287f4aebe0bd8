#!/usr/bin/env python3
"""Smoothing of diarized turns on the device (smooth.py, csrc/smooth.hip) on one MI355X -> one JSON line.

For 256 x 3 min and for one hour of tools/der_bench.py's generated hypothesis tables (4 speakers, rows of every kind) on the packed frame
grid, at min_duration_off = 0.1 and 0.5 s and min_duration_on = 0 and 0.25 s:
  device path      backend.smooth_diarization's work (smooth.smooth_results: one upload, sdk_smooth_turns's three launches, one download, the
                   turns cut on the host) beside smooth.smooth_host over the same pack in the same process (wall clock, minimum and median
                   of --iters windows after a warm-up), and whether table and tallies agree
  launches         the device time of sdk_smooth_turns alone on resident tables (a window of WINDOW back-to-back calls between two events,
                   divided by WINDOW; the copy of the table that smooth.smooth_turns makes first is inside) and, as a bandwidth yardstick,
                   that of sdk_score_cooccur over the same frames (it reads 17 bytes per frame once; sdk_smooth_turns moves 64 bytes per
                   frame through its three launches, the walks aside); once more at fill = keep = MAX_SMOOTH_FRAMES, the longest walks
  sweep            --sweep-config RxSECONDS of der_bench's generated audio, --thresholds T thresholds: Diarizer.sweep with the four pairs
                   beside the sweep without the keyword, minimum and median of --iters windows each, and the waits per pack of both
Record the line in profiles/r37_smooth_bench.json.
    python tools/smooth_bench.py [--iters 3] [--sweep-config 16x180] [--thresholds 4]"""
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
PAIRS = [(0.1, 0.0), (0.1, 0.25), (0.5, 0.0), (0.5, 0.25)]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--sweep-config", default="16x180", help="RxSECONDS, or 'none'")
    ap.add_argument("--thresholds", type=int, default=4)
    args = ap.parse_args()
    iters = max(args.iters, 3)
    import torch
    from der_bench import hypothesis, recording, reference, windows
    ops, sm, sc, dz, seg, rn = (importlib.import_module(f"{PKG}.{m}") for m in ("ops", "smooth", "score", "diarize", "segmentation", "resnet"))
    lib = importlib.import_module(f"{PKG}._lib")
    eng = ops.get_engine(0)

    def device_ms(fn):
        fn()
        torch.cuda.synchronize()
        best = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(WINDOW):
                fn()
            b.record()
            torch.cuda.synchronize()
            best.append(a.elapsed_time(b) / WINDOW)
        return round(min(best), 4)

    out = {"tool": "smooth_bench", "device": lib.device_info(0)["name"], "iters": iters, "window": WINDOW, "configs": {}, "sweep": None}
    for name, R, secs in CONFIGS:
        G = dz.global_frames(int(secs * 16000))
        results = [SimpleNamespace(speakers=hypothesis(1000 + r, G), n_speakers=4) for r in range(R)]
        sp = np.concatenate([res.speakers for res in results])
        frame_off, cent_off = np.arange(R + 1, dtype=np.int64) * G, np.arange(R + 1, dtype=np.int64) * 4
        tab = dz.GroupTables(eng, np.zeros(R + 1, np.int64), frame_off, [270 * G + 226] * R).set_clusters(cent_off)
        sp_d = torch.from_numpy(sp).to(eng.device)
        cfg = {"recordings": R, "frames": R * G, "pairs": []}
        for off, on in PAIRS:
            fill, keep = sm.fill_frames_of(off), sm.keep_frames_of(on)
            got = sm.smooth_results(eng, results, off, on)
            want, tal = sm.smooth_host(sp, frame_off, cent_off, fill, keep, 2)
            _, t_dev = windows(lambda: sm.smooth_results(eng, results, off, on), iters)
            _, t_host = windows(lambda: sm.smooth_host(sp, frame_off, cent_off, fill, keep, 2), iters)
            cfg["pairs"].append({"min_duration_off": off, "min_duration_on": on, "fill": fill, "keep": keep, "filled": int(tal[:, 0].sum()),
                                 "dropped": int(tal[:, 1].sum()), "device_path": t_dev, "smooth_host": t_host,
                                 "speedup_min": round(t_host["min_s"] / t_dev["min_s"], 2),
                                 "agree": bool(np.array_equal(np.concatenate([g.speakers for g in got]), want)
                                               and [[g.smoothing["filled"], g.smoothing["dropped"]] for g in got] == tal.tolist()),
                                 "device_smooth_turns_ms": device_ms(lambda: sm.smooth_turns(eng, sp_d, tab, fill, keep, 2))})
        cfg["device_smooth_turns_longest_walks_ms"] = device_ms(lambda: sm.smooth_turns(eng, sp_d, tab, sm.MAX_SMOOTH_FRAMES, sm.MAX_SMOOTH_FRAMES, 2))
        pref = sc.rasterise_references(eng, tab, [[(0.0, secs, "a")] for _ in range(R)])
        co_s, tally_s = torch.empty((R * 4,), dtype=torch.int32, device=eng.device), torch.empty((R, 5), dtype=torch.int64, device=eng.device)
        co_off_s = torch.arange(R + 1, dtype=torch.int64, device=eng.device) * 4
        cfg["device_score_cooccur_ms"] = device_ms(lambda: lib.check(eng.lib.sdk_score_cooccur(
            eng.ctx, pref.ref_mask.data_ptr(), pref.scored.data_ptr(), sp_d.data_ptr(), tab.frame_off_d.data_ptr(), pref.ref_off_d.data_ptr(),
            tab.cent_off_d.data_ptr(), co_off_s.data_ptr(), R, tab.G, pref.max_ref, 4, R * 4, co_s.data_ptr(), tally_s.data_ptr(), None), "sdk_score_cooccur"))
        cfg["bytes_moved_smooth_turns"] = int(R * G * (8 + 8 + 8 + 16 + 16 + 8 + 8 + 8))      # the copy, then each launch's own read and write per frame
        cfg["bytes_read_score_cooccur"] = int(17 * R * G)
        out["configs"][name] = cfg
    if args.sweep_config != "none":
        R, secs = (int(v) for v in args.sweep_config.split("x"))
        ths = [round(float(t), 4) for t in np.linspace(0.3, 1.2, args.thresholds)]
        diar = dz.Diarizer(eng, seg.Segmentation(eng, seg.synthetic_weights(0)), rn.ResNet34(eng, rn.synthetic_weights(0)))
        recs = [recording(r, secs * 16000) for r in range(R)]
        refs = [reference(r, secs) for r in range(R)]
        kw = dict(step_s=1.0, constrained=True)
        diar.sweep(recs[:2], refs[:2], ths[:2], smoothing=PAIRS[:1], **kw)       # warm-up: code objects, scratch buffers
        plain, t_plain = windows(lambda: diar.sweep(recs, refs, ths, **kw), iters)
        sync_plain = [dict(s) for s in diar.last_sync]
        four, t_four = windows(lambda: diar.sweep(recs, refs, ths, smoothing=PAIRS, **kw), iters)
        out["sweep"] = {"recordings": R, "seconds_each": secs, "thresholds": ths, "pairs": PAIRS, "sweep_plain": t_plain, "sweep_four_pairs": t_four,
                        "four_pairs_over_plain_min": round(t_four["min_s"] / t_plain["min_s"], 3), "waits_per_pack_plain": sync_plain[0],
                        "waits_per_pack_four_pairs": dict(diar.last_sync[0]), "pooled_der_plain": [round(p.der, 4) for p in plain.pooled],
                        "pooled_der_four_pairs": [[round(p.der, 4) for p in row] for row in four.pooled], "best": list(four.best)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
