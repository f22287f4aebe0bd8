#!/usr/bin/env python3
"""Diarization of one hour at a 1-s step (3 591 ten-second chunks): one JSON line with the per-stage split (warm, event-timed on the
device; clustering / assignment / reconstruction / host by wall clock), chunks/s, the real-time factor, and two yardsticks timed in the same
process on the same inputs:
  trunk sharing   three ResNet34.forward calls per chunk at T = 1001 (what embedding each (chunk, speaker) pair separately costs) against
                  the one masked forward; the ratio is reported, not gated
  reconstruction  the numpy statement of the stitching rule (diarize.reconstruct_host) on the same class table
  assignment      the constrained stage on the device (training rows and labels up, sdk_diarize_centroids + sdk_diarize_assign, labels, scores
                  and centroids down; wall clock, best of three after a warm-up) beside the host stage it stands in for (the download of
                  the embeddings + diarize.assign_rows) on the same embeddings, and how many chunks the constraint changed
Record the line in profiles/r11_diarize_assign_bench.json (r10_diarize_bench.json: the line before the constrained stage).  Synthetic weights: the class table is the model's own (noise-like) output, which
exercises every stage at full size."""
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--step", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--no-yardstick", action="store_true")
    a = ap.parse_args()
    import torch
    ops = importlib.import_module(f"{PKG}.ops")
    seg = importlib.import_module(f"{PKG}.segmentation")
    rn = importlib.import_module(f"{PKG}.resnet")
    dz = importlib.import_module(f"{PKG}.diarize")
    cluster = importlib.import_module(f"{PKG}.cluster")
    eng = ops.get_engine(0)
    model, net = seg.Segmentation(eng, seg.synthetic_weights(0)), rn.ResNet34(eng, rn.synthetic_weights(0))
    n = int(a.seconds * 16000)
    rng = np.random.default_rng(0)
    x = np.clip(np.round(rng.normal(0, 0.1, n) * (1 + np.sin(2 * np.pi * 0.3 * np.arange(n) / 16000)) * 32768), -32768, 32767).astype(np.int16)
    st = seg.chunk_starts(n, a.step)
    Cn, F, T = len(st), seg.num_frames(seg.CHUNK), ops.num_frames(seg.CHUNK)
    T4 = net.last_map_frames(T)
    rec = torch.from_numpy(x).cuda()
    sd = torch.from_numpy(st.astype(np.int32)).cuda()
    stages = ["segmentation", "decode_masks", "fbank", "trunk_pool_seg1", "l2norm"]

    def device_pass(timed: bool):
        ev = {k: 0.0 for k in stages}
        cls = torch.empty((Cn, F), dtype=torch.uint8, device="cuda")
        infos, embs = [], []
        for b0 in range(0, Cn, a.batch):
            s = sd[b0:b0 + a.batch]
            B = int(s.numel())
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            marks[0].record()
            lp = model.forward(rec, s)
            marks[1].record()
            c = dz.powerset_decode(eng, lp)
            w, info = dz.diarize_masks(eng, c, T4)
            valid = info[:, :, 3].contiguous()
            marks[2].record()
            feats = eng.fbank_windows(rec.data_ptr(), n, s.data_ptr(), B, seg.CHUNK)
            marks[3].record()
            emb = net.forward_masked(feats, B, T, w, valid)
            marks[4].record()
            E = eng.l2norm(emb)[0]
            marks[5].record()
            cls[b0:b0 + B] = c
            infos.append(info)
            embs.append(E)
            if timed:
                torch.cuda.synchronize()
                for i, k in enumerate(stages):
                    ev[k] += marks[i].elapsed_time(marks[i + 1])
        torch.cuda.synchronize()
        return ev, cls, torch.cat(infos), torch.cat(embs)

    device_pass(False)                                                    # warm-up: scratch buffers, code objects
    best = None
    for _ in range(a.iters):
        t0 = time.perf_counter()
        ev, cls, info_d, E_d = device_pass(True)
        ev["device_wall"] = (time.perf_counter() - t0) * 1e3
        if best is None or ev["device_wall"] < best[0]["device_wall"]:
            best = (ev, cls, info_d, E_d)
    ev, cls, info_d, E_d = best
    # the pooling + seg_1 share of the masked forward: the profile of one batch
    B = min(a.batch, Cn)
    feats = eng.fbank_windows(rec.data_ptr(), n, sd[:B].data_ptr(), B, seg.CHUNK)
    w, info = dz.diarize_masks(eng, cls[:B].contiguous(), T4)
    eng.profile_begin()
    net.forward_masked(feats, B, T, w, info[:, :, 3].contiguous())
    torch.cuda.synchronize()
    prof = eng.profile_end()
    tail = sum(v["ms"] for k, v in prof.items() if k in ("resnet_pool", "rows_fc", "copy"))
    total = sum(v["ms"] for v in prof.values())
    t0 = time.perf_counter()
    info = info_d.cpu().numpy()
    E = E_d.cpu().numpy()
    E[info.reshape(-1, 4)[:, 3] == 0] = 0.0
    train = dz.training_rows(info, F)
    t_host = time.perf_counter() - t0
    t0 = time.perf_counter()
    tl = cluster.agglomerative_cluster(eng, E_d.index_select(0, torch.from_numpy(train).cuda()).contiguous(), a.threshold, 12).labels if len(train) > 1 \
        else np.zeros(len(train), np.int32)
    t_cluster = time.perf_counter() - t0
    t0 = time.perf_counter()
    labels, cent = dz.assign_rows(E, info, train, tl)
    t_assign = time.perf_counter() - t0
    constrained = None
    if len(train):
        def device_stage():
            c32, c64 = dz.diarize_centroids(eng, E_d, torch.from_numpy(train.astype(np.int32)).cuda(), torch.from_numpy(np.asarray(tl, dtype=np.int32)).cuda(),
                                            int(np.max(tl)) + 1)
            lab, sc = dz.diarize_assign(eng, E_d, info_d.contiguous(), c64, True)
            return lab.cpu().numpy(), sc.cpu().numpy(), c32.cpu().numpy()
        device_stage()
        t_dev = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lab_c, _, cent_c = device_stage()
            t_dev.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        E_again = E_d.cpu().numpy()
        t_down = time.perf_counter() - t0
        del E_again
        constrained = {"device_stage_ms": round(min(t_dev) * 1e3, 3), "host_assign_rows_ms": round(t_assign * 1e3, 3),
                       "host_embedding_download_ms": round(t_down * 1e3, 3),
                       "chunks_changed_by_the_constraint": int((lab_c != labels).any(1).sum()),
                       "candidates_dropped": int(((lab_c < 0) & (labels >= 0)).sum()),
                       "centroids_max_abs_diff": float(np.abs(cent_c - cent).max())}
    K = max(cent.shape[0], 1)
    lab_d = torch.from_numpy(labels).cuda()
    dz.diarize_reconstruct(eng, cls, sd, lab_d, K, n)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    count, speakers, _ = dz.diarize_reconstruct(eng, cls, sd, lab_d, K, n)
    count, speakers = count.cpu().numpy(), speakers.cpu().numpy()
    t_rec = time.perf_counter() - t0
    t0 = time.perf_counter()
    turns = dz.turns_from_frames(speakers, cent.shape[0])
    t_host += time.perf_counter() - t0
    total_s = ev["device_wall"] / 1e3 + t_host + t_cluster + t_assign + t_rec
    out = {"tool": "diarize_bench", "seconds": a.seconds, "step_s": a.step, "chunks": Cn, "batch": a.batch, "T": T, "T4": T4,
           "stage_ms": {**{k: round(v, 2) for k, v in ev.items()}, "clustering": round(t_cluster * 1e3, 2), "assignment": round(t_assign * 1e3, 2),
                        "reconstruction": round(t_rec * 1e3, 2), "host": round(t_host * 1e3, 2)},
           "masked_pool_seg1_share_of_forward": round(tail / total, 4) if total else None,
           "total_s": round(total_s, 4), "chunks_per_s": round(Cn / total_s, 1), "real_time_factor": round(total_s / a.seconds, 7),
           "training_rows": int(len(train)), "clusters": int(cent.shape[0]), "turns": len(turns)}
    if constrained is not None:
        out["constrained_assignment"] = constrained
    if not a.no_yardstick:
        t_three = 0.0
        for b0 in range(0, Cn, a.batch):
            s = sd[b0:b0 + a.batch]
            B = int(s.numel())
            feats = eng.fbank_windows(rec.data_ptr(), n, s.data_ptr(), B, seg.CHUNK)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(3):
                net.forward(feats, B, T)
            e1.record()
            torch.cuda.synchronize()
            t_three += e0.elapsed_time(e1)
        cls_h = cls.cpu().numpy()
        t0 = time.perf_counter()
        rc, rs, _, _ = dz.reconstruct_host(cls_h, st, labels, K, n)
        t_np = time.perf_counter() - t0
        out["yardsticks"] = {"three_forwards_per_chunk_ms": round(t_three, 2), "masked_forward_ms": round(ev["trunk_pool_seg1"], 2),
                             "embedding_stage_ratio": round(ev["trunk_pool_seg1"] / t_three, 4),
                             "reconstruction_numpy_ms": round(t_np * 1e3, 2), "reconstruction_gpu_ms": round(t_rec * 1e3, 2),
                             "reconstruction_equal": bool(np.array_equal(rc, count) and np.array_equal(rs, speakers))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
