#!/usr/bin/env python3
"""Diarization of one hour at a 1-s step (3 591 ten-second chunks): one JSON line with the per-stage split (warm, event-timed on the
device; clustering / assignment / reconstruction / host by wall clock), chunks/s, the real-time factor, and two yardsticks timed in the same
process on the same inputs:
  trunk sharing   three ResNet34.forward calls per chunk at T = 1001 (what embedding each (chunk, speaker) pair separately costs) against
                  the one masked forward; the ratio is reported, not gated
  reconstruction  the numpy statement of the stitching rule (diarize_host.reconstruct_host) on the same class table
  assignment      the constrained stage on the device (training rows and labels up, sdk_diarize_centroids + sdk_diarize_assign, labels, scores
                  and centroids down; wall clock, best of three after a warm-up) beside the host stage it stands in for (the download of
                  the embeddings + diarize_host.assign_rows) on the same embeddings, and how many chunks the constraint changed
  vbx             the VBx clustering's device stretch (sdk_plda_transform + sdk_vbx, all iterations enqueued + sdk_vbx_centroids; wall clock
                  around ONE final synchronisation, best of three after a warm-up) on two inputs - the hour's training rows with the initial
                  labels of the linkage's cut at 0.6, and a generated table of N = 10 000 rows, D = 128, with 5 true speakers split into 50
                  initial clusters (the synthetic weights yield one cluster, which exercises nothing) - beside a vectorised numpy restatement
                  of the same rule on the same input, with at most 16 threads.  Record the line in profiles/r12_vbx_bench.json.
Record the line in profiles/r11_diarize_assign_bench.json (r10_diarize_bench.json: the line before the constrained stage).  Synthetic weights: the class table is the model's own (noise-like) output, which
exercises every stage at full size."""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time
from pathlib import Path

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):          # the numpy yardsticks: at most 16 threads
    os.environ[_v] = str(min(16, int(os.environ.get(_v, "16") or 16)))
import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PKG = "speaker-diarization-toolkit_amd"


def vbx_numpy(plda, E, init, S, Fa=0.07, Fb=0.8, max_iters=20, epsilon=1e-4, init_smoothing=7.0):
    """cluster.vbx_cluster's transform, iteration and centroids in vectorised numpy (float64) -> (n_iter, kept speakers, unit centroids)."""
    X = plda.transform_host(E)
    Phi = plda.Phi
    n, D = X.shape
    rho = X * np.sqrt(Phi)
    G = -0.5 * ((X ** 2).sum(1) + D * np.log(2 * np.pi))
    a = np.where(np.arange(S)[None, :] == np.asarray(init)[:, None], 0.0, -init_smoothing)
    gamma = np.exp(a) / np.exp(a).sum(1, keepdims=True)
    pi = np.full(S, 1.0 / S)
    prev, n_iter = None, 0
    for ii in range(max_iters):
        invL = 1.0 / (1.0 + Fa / Fb * gamma.sum(0)[:, None] * Phi)
        alpha = Fa / Fb * invL * (gamma.T @ rho)
        with np.errstate(divide="ignore"):
            z = Fa * (rho @ alpha.T - 0.5 * ((invL + alpha ** 2) @ Phi)[None, :] + G[:, None]) + np.log(pi)
        m = z.max(1, keepdims=True)
        lse = m[:, 0] + np.log(np.exp(z - m).sum(1))
        gamma = np.exp(z - lse[:, None])
        elbo = lse.sum() + 0.5 * Fb * (np.log(invL) - invL - alpha ** 2 + 1).sum()
        pi = gamma.sum(0) / gamma.sum()
        n_iter = ii + 1
        if ii > 0 and elbo - prev < epsilon:
            break
        prev = elbo
    keep = np.flatnonzero(pi > 1e-7)
    g = gamma[:, keep]
    cent = (g.T @ E.astype(np.float64)) / g.sum(0)[:, None]
    return n_iter, keep, cent / np.linalg.norm(cent, axis=1, keepdims=True)


def vbx_table(plda_mod, N=10000, d_in=256, D0=128, D=128, S=50, n_true=5, seed=0):
    """A generated table: n_true speaker means at scale sqrt(Phi) in PLDA space, rows N(mean, I), carried back to unit fp32 embeddings through
    the inverse of the transform's linear parts; every speaker's rows dealt to its S / n_true initial clusters in turn."""
    m = plda_mod.synthetic_plda(d_in, D0, seed, D)
    Phi_full, T_full = plda_mod.prepare(m.tr, m.psi, D0)
    rng = np.random.default_rng(seed)
    true = rng.integers(0, n_true, N)
    x = (rng.standard_normal((n_true, D0)) * np.sqrt(Phi_full))[true] + rng.standard_normal((N, D0))

    def on_sphere(centre, dirs, radius):
        u = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
        b = u @ centre
        return centre[None, :] + (-b + np.sqrt(b * b + radius * radius - centre @ centre))[:, None] * u
    y = m.mu[None, :] + x @ np.linalg.inv(T_full).T
    E = on_sphere(m.mean1, on_sphere(m.mean2, y, np.sqrt(d_in)) @ m.lda.T, 1.0).astype(np.float32)
    init = np.zeros(N, np.int32)
    for v in range(n_true):
        idx = np.flatnonzero(true == v)
        init[idx] = np.arange(v, S, n_true)[np.arange(len(idx)) % len(np.arange(v, S, n_true))]
    return m, E, init


def vbx_leg(eng, torch, plda, E_d, rows, init, S):
    """Device time of transform + VBx + centroids (ms, best of three, one synchronisation) and the numpy restatement's on the same input."""
    rows_d = torch.from_numpy(np.asarray(rows, dtype=np.int32)).cuda()
    init_d = torch.from_numpy(np.asarray(init, dtype=np.int32)).cuda()
    Phi = plda.device_arrays(E_d.device)["Phi"]

    def stage():
        X = eng.plda_transform(E_d, rows_d, plda, check_rows=False)
        gamma, pi, elbo, n_iter, status = eng.vbx(X, Phi, init_d, S)
        out = eng.vbx_centroids(gamma, pi, E_d, rows_d, check_rows=False)
        torch.cuda.synchronize()
        return n_iter, status, out
    stage()
    t_dev = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_iter, status, (K, keep, _, _, c64) = stage()
        t_dev.append(time.perf_counter() - t0)
    Eh = E_d.cpu().numpy()[np.asarray(rows)]
    t0 = time.perf_counter()
    n_np, keep_np, cent_np = vbx_numpy(plda, Eh, init, S)
    t_np = time.perf_counter() - t0
    Kn = int(K.item())
    same = Kn == len(keep_np) and np.array_equal(keep.cpu().numpy()[:Kn], keep_np)
    return {"rows": int(len(rows)), "D": int(plda.lda_dim), "d_in": int(plda.d_in), "initial_speakers": int(S), "kept_speakers": Kn,
            "n_iter": int(n_iter.item()), "status": int(status.item()), "device_ms": round(min(t_dev) * 1e3, 3), "numpy_ms": round(t_np * 1e3, 3),
            "numpy_n_iter": int(n_np), "numpy_threads": int(os.environ["OMP_NUM_THREADS"]), "same_kept_speakers": bool(same),
            "centroids_max_abs_diff": float(np.abs(c64.cpu().numpy()[:Kn] - cent_np).max()) if same else None}


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
    plda_mod = importlib.import_module(f"{PKG}.plda")
    vbx = {}
    if len(train) > 1:
        Z = eng.centroid_linkage(E_d.index_select(0, torch.from_numpy(train).cuda()).contiguous()).cpu().numpy()
        init = cluster.fcluster_distance(Z, cluster.VBX_AHC_THRESHOLD)
        vbx["hour"] = vbx_leg(eng, torch, plda_mod.synthetic_plda(E_d.shape[1], 128, 0), E_d, train, init, int(init.max()) + 1)
    m_t, E_t, init_t = vbx_table(plda_mod)
    vbx["table"] = vbx_leg(eng, torch, m_t, torch.from_numpy(E_t).cuda(), np.arange(len(E_t)), init_t, 50)
    out["vbx"] = vbx
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
