#!/usr/bin/env python3
"""Speaker-attributed transcripts on the device (words.py, csrc/words.hip) on one MI355X -> one JSON line.

For every configuration - 256 x 3 min of about 450 words each, one hour of about 9 000 words, and the hour cut into 30-s spans (the
long-span path: about 1 780 frames per "word") - generated hypothesis tables (4 speakers, rows of every kind) on the packed frame grid and
generated words with reference labels:
  attribute        words.attribute - host preparation, uploads, the one launch and the one download - beside a loop of words.attribute_host
                   over the same recordings in the same process (wall clock, minimum and median of --iters windows after a warm-up), and
                   whether every row agrees
  wder             words.wder_pack on the attributed pack (sdk_words_cooccur + sdk_score_map and the one download) beside a loop of
                   words.wder_host, and whether every tally agrees
  device           the device time of sdk_words_attribute alone and of sdk_words_cooccur + sdk_score_map alone (a window of WINDOW
                   back-to-back calls between two events, divided by WINDOW), and as a bandwidth yardstick that of sdk_score_cooccur over
                   the same frames (it reads 17 bytes per frame once; sdk_words_attribute reads 8 bytes per frame of every word)
Record the line in profiles/r33_words_bench.json.
    python tools/words_bench.py [--iters 3]"""
from __future__ import annotations

import argparse
import importlib
import json
import statistics
import sys
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PKG = "speaker-diarization-toolkit_amd"
WINDOW = 20
CONFIGS = [("256x180s", 256, 180.0, 450, None), ("1x3600s", 1, 3600.0, 9000, None), ("1x3600s_30s_spans", 1, 3600.0, 0, 30.0)]


def hypothesis(seed: int, G: int, K: int = 4) -> np.ndarray:
    rng = np.random.default_rng(seed)
    sp = np.full((G, 2), -1, np.int32)
    first = np.repeat(rng.integers(-1, K, G // 40 + 1), 40)[:G]
    second = np.repeat(rng.integers(-1, K, G // 40 + 1), 40)[:G]
    sp[:, 0] = first
    ok = (first >= 0) & (second >= 0) & (second != first) & (rng.uniform(size=G) < 0.2)
    sp[ok, 1] = second[ok]
    return sp


def words_of(seed: int, secs: float, n: int, span):
    """n words of 0.1 - 0.6 s spread over the recording, or back-to-back spans of `span` seconds; labels over 3 names."""
    rng = np.random.default_rng(seed)
    if span:
        starts = np.arange(0.0, secs, span)
        out = [(float(s), float(min(s + span, secs))) for s in starts]
    else:
        starts = np.sort(rng.uniform(0.0, secs - 0.7, n))
        out = [(float(round(s, 3)), float(round(s + rng.uniform(0.1, 0.6), 3))) for s in starts]
    return out, [f"s{int(k)}" for k in rng.integers(0, 3, len(out))]


def timed(fn, iters: int):
    fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"min_ms": round(min(ts) * 1e3, 3), "median_ms": round(statistics.median(ts) * 1e3, 3)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    args = ap.parse_args()
    import torch
    ops, wd, sc, dz, ops_score = (importlib.import_module(f"{PKG}.{m}") for m in ("ops", "words", "score", "diarize", "ops_score"))
    lib = importlib.import_module(f"{PKG}._lib")
    eng = ops.get_engine(0)
    gap = wd.gap_frames(0.5)

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

    out = {"tool": "words_bench", "device": lib.device_info(0)["name"], "iters": args.iters, "window": WINDOW, "gap_frames": gap, "configs": {}}
    for name, R, secs, n_words, span in CONFIGS:
        G = dz.global_frames(int(secs * 16000))
        results = [SimpleNamespace(speakers=hypothesis(1000 + r, G), n_speakers=4) for r in range(R)]
        both = [words_of(2000 + r, secs, n_words, span) for r in range(R)]
        words, refs = [w for w, _ in both], [l for _, l in both]
        samples = [wd.prepare_words(w) for w in words]
        W = sum(len(w) for w in words)
        cfg = {"recordings": R, "frames": R * G, "words": W}
        labels = wd.attribute(eng, results, words)
        host = [wd.attribute_host(res.speakers, 4, s, gap) for res, s in zip(results, samples)]
        cfg["rows_agree"] = all(np.array_equal(a.rows, b) for a, b in zip(labels, host))
        cfg["frames_per_word"] = round(float(np.concatenate([h[:, 3] for h in host]).mean()), 1)
        cfg["attribute"] = timed(lambda: wd.attribute(eng, results, words), args.iters)
        cfg["attribute_host"] = timed(lambda: [wd.attribute_host(res.speakers, 4, s, gap) for res, s in zip(results, samples)], args.iters)
        pack = wd.attribute_pack(eng, results, words)
        got = wd.wder_pack(eng, pack, refs)
        want = [wd.wder_host(h[:, 0], l, 4) for h, l in zip(host, refs)]
        cfg["wder_agree"] = all((a.scored, a.unassigned, a.correct) == (b.scored, b.unassigned, b.correct) and np.array_equal(a.co, b.co) for a, b in zip(got, want))
        cfg["wder_pooled"] = round(wd.pool(got).wder, 6)
        cfg["wder"] = timed(lambda: wd.wder_pack(eng, pack, refs), args.iters)
        cfg["wder_host"] = timed(lambda: [wd.wder_host(h[:, 0], l, 4) for h, l in zip(host, refs)], args.iters)
        # the kernels alone, on resident tables
        tab = dz.GroupTables(eng, np.zeros(R + 1, np.int64), np.arange(R + 1, dtype=np.int64) * G, [270 * G + 226] * R)
        tab.set_clusters(np.arange(R + 1, dtype=np.int64) * 4)
        sp_d = torch.from_numpy(np.concatenate([res.speakers for res in results])).to(eng.device)
        words_d = torch.from_numpy(np.concatenate(samples)).to(eng.device)
        ids = [wd._reference_ids(l) for l in refs]
        ref_d = torch.from_numpy(np.concatenate([i for i, _ in ids])).to(eng.device)
        S_r = np.asarray([len(n) for _, n in ids], np.int64)
        ref_off = np.concatenate([[0], np.cumsum(S_r)])
        co_off = np.concatenate([[0], np.cumsum(S_r * 4)]).astype(np.int64)
        ref_off_d, co_off_d = torch.from_numpy(ref_off.astype(np.int32)).to(eng.device), torch.from_numpy(co_off).to(eng.device)
        mapping = torch.empty((int(ref_off[-1]),), dtype=torch.int32, device=eng.device)
        correct = torch.empty((R,), dtype=torch.int64, device=eng.device)

        def cooccur_map():
            co, _ = ops_score.words_cooccur(eng, pack.rows, ref_d, pack.word_off_d, ref_off_d, tab.cent_off_d, co_off_d, int(S_r.max()), 4, int(co_off[-1]))
            lib.check(eng.lib.sdk_score_map(eng.ctx, co.data_ptr(), ref_off_d.data_ptr(), tab.cent_off_d.data_ptr(), co_off_d.data_ptr(), R, int(S_r.max()), 4,
                                            mapping.data_ptr(), correct.data_ptr(), None), "sdk_score_map")

        cfg["device_attribute_ms"] = device_ms(lambda: ops_score.words_attribute(eng, words_d, pack.word_off_d, sp_d, tab.frame_off_d, tab.cent_off_d, 4, gap))
        cfg["device_cooccur_map_ms"] = device_ms(cooccur_map)
        pref = sc.rasterise_references(eng, tab, [[(0.0, secs, "a")] for _ in range(R)])
        co_s, tally_s = torch.empty((R * 4,), dtype=torch.int32, device=eng.device), torch.empty((R, 5), dtype=torch.int64, device=eng.device)
        co_off_s = torch.arange(R + 1, dtype=torch.int64, device=eng.device) * 4
        cfg["device_score_cooccur_ms"] = device_ms(lambda: lib.check(eng.lib.sdk_score_cooccur(
            eng.ctx, pref.ref_mask.data_ptr(), pref.scored.data_ptr(), sp_d.data_ptr(), tab.frame_off_d.data_ptr(), pref.ref_off_d.data_ptr(),
            tab.cent_off_d.data_ptr(), co_off_s.data_ptr(), R, tab.G, pref.max_ref, 4, R * 4, co_s.data_ptr(), tally_s.data_ptr(), None), "sdk_score_cooccur"))
        cfg["bytes_read_attribute"] = int(8 * sum(int(h[:, 3].sum()) for h in host) + 8 * W)
        out["configs"][name] = cfg
    print(json.dumps(out))


if __name__ == "__main__":
    main()
