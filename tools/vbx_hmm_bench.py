#!/usr/bin/env python3
"""Device time of VBx with its HMM (sdk_vbx_hmm) beside the mixture (sdk_vbx) on the same input, and beside numpy.

An hour at a 0.25-s step: n = 14 400 rows in time order (speaker runs), D = 128, S in {8, 32, 130} initial speakers.  Both calls run a FIXED
number of iterations (epsilon = -inf, --iters), so the times compare like with like; each is timed with device events around the one call
(all launches enqueued, no host synchronisation inside), --warmup calls first, then --repeats calls: the median and the minimum are reported.

  hmm_ms, vbx_ms            one call, all iterations
  chain_us_per_step         (hmm_ms - vbx_ms) / (iters * n): what the HMM adds per row and iteration.  The two passes run side by side in one
                            launch, so this is the cost of ONE dependent step (plus the logp store and the post kernel's share), not of two.
  hmm_us_per_step           hmm_ms / (iters * n): the whole iteration charged to the chain, an upper bound
  numpy_ms_per_iter         the same rule in numpy, vectorised over the speakers, the rows in a Python loop (a chain has no other form there);
                            one iteration, at most 16 threads

Prints one JSON line; the record is profiles/r18_vbx_hmm_bench.json."""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time
from pathlib import Path

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):          # the numpy yardstick: at most 16 threads
    os.environ[_v] = str(min(16, int(os.environ.get(_v, "16") or 16)))
import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PKG = "speaker-diarization-toolkit_amd"


def sequence(n, D, S, n_true=4, seed=0, mean_run=12):
    """X [n, D] in PLDA space, rows in speaker runs of 1 .. 2 mean_run; Phi [D]; init [n]: every speaker's rows dealt to its initial clusters."""
    rng = np.random.default_rng(seed)
    Phi = np.geomspace(16.0, 0.05, D)
    means = rng.standard_normal((n_true, D)) * np.sqrt(Phi)
    true = np.zeros(n, np.int64)
    t, last = 0, -1
    while t < n:
        v = int(rng.integers(n_true - 1))
        v += last >= 0 and v >= last
        k = int(rng.integers(1, 2 * mean_run + 1))
        true[t:t + k] = v
        t, last = t + k, v
    X = means[true] + rng.standard_normal((n, D))
    init = np.zeros(n, np.int32)
    for v in range(n_true):
        mine = np.arange(v, S, n_true) if v < S else np.array([v % S])
        idx = np.flatnonzero(true == v)
        init[idx] = mine[np.arange(len(idx)) % len(mine)]
    return X, Phi, init


def hmm_numpy_iteration(X, Phi, gamma, pi, P, Fa=0.07, Fb=0.8):
    """One iteration of cluster.vbx_cluster's HMM rule in numpy -> (gamma, pi, elbo)."""
    n, D = X.shape
    rho = X * np.sqrt(Phi)
    G = -0.5 * ((X ** 2).sum(1) + D * np.log(2 * np.pi))
    invL = 1.0 / (1.0 + Fa / Fb * gamma.sum(0)[:, None] * Phi)
    alpha = Fa / Fb * invL * (gamma.T @ rho)
    logp = Fa * (rho @ alpha.T - 0.5 * ((invL + alpha ** 2) @ Phi)[None, :] + G[:, None])
    with np.errstate(divide="ignore"):
        lnP, ln1mP, lnpi = np.log(P), np.log1p(-P), np.log(pi)
    lf, lb, m = np.empty_like(logp), np.zeros_like(logp), np.empty(n)

    def lse(u):
        mx = u.max()
        return mx + np.log(np.exp(u - mx).sum())
    lf[0] = logp[0] + lnpi
    for t in range(1, n):
        m[t - 1] = lse(lf[t - 1])
        lf[t] = logp[t] + np.logaddexp(lnP + lf[t - 1], ln1mP + lnpi + m[t - 1])
    m[n - 1] = lse(lf[n - 1])
    for t in range(n - 2, -1, -1):
        q = logp[t + 1] + lb[t + 1]
        lb[t] = np.logaddexp(lnP + q, ln1mP + lse(lnpi + q))
    tll = m[n - 1]
    gamma = np.exp(lf + lb - tll)
    pinew = gamma[0] + (1.0 - P) * pi * np.exp(m[:-1, None] + logp[1:] + lb[1:] - tll).sum(0)
    return gamma, pinew / pinew.sum(), tll + 0.5 * Fb * (np.log(invL) - invL - alpha ** 2 + 1).sum()


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=14400)
    ap.add_argument("--speakers", type=int, nargs="+", default=[8, 32, 130])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--loop-prob", type=float, default=0.99)
    args = ap.parse_args()
    import torch
    ops = importlib.import_module(f"{PKG}.ops")
    lib = importlib.import_module(f"{PKG}._lib")
    eng = ops.get_engine(0)
    D, n, P = 128, args.n, args.loop_prob
    out = {"tool": "vbx_hmm_bench", "device": lib.device_info(0)["name"], "n": n, "D": D, "loop_prob": P, "iters": args.iters, "warmup": args.warmup,
           "repeats": args.repeats, "numpy_threads": int(os.environ["OMP_NUM_THREADS"]), "cases": []}
    for S in args.speakers:
        X, Phi, init = sequence(n, D, S)
        Xd, Phid, initd = (torch.from_numpy(a).cuda() for a in (X, Phi, init))
        kw = dict(max_iters=args.iters, epsilon=float("-inf"))
        calls = {"hmm": lambda: eng.vbx_hmm(Xd, Phid, initd, S, P, **kw), "vbx": lambda: eng.vbx(Xd, Phid, initd, S, **kw)}
        ms, res = {}, {}
        for name, call in calls.items():
            for _ in range(args.warmup):
                call()
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                res[name] = call()
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b))
            ms[name] = ts
        n_it = {k: int(v[3].item()) for k, v in res.items()}
        st = {k: int(v[4].item()) for k, v in res.items()}
        a = np.zeros((n, S))
        a[np.arange(n), init] = 7.0
        g0 = np.exp(a - 7.0)
        g0 /= g0.sum(1, keepdims=True)
        t0 = time.perf_counter()
        g1, pi1, e1 = hmm_numpy_iteration(X, Phi, g0, np.full(S, 1.0 / S), P)
        t_np = time.perf_counter() - t0
        e_dev = float(res["hmm"][2][0].item())
        hmm, vbx = float(np.median(ms["hmm"])), float(np.median(ms["vbx"]))
        steps = args.iters * n
        out["cases"].append({"S": S, "hmm_ms": round(hmm, 3), "hmm_ms_min": round(min(ms["hmm"]), 3), "vbx_ms": round(vbx, 3),
                             "vbx_ms_min": round(min(ms["vbx"]), 3), "chain_us_per_step": round((hmm - vbx) * 1e3 / steps, 4),
                             "hmm_us_per_step": round(hmm * 1e3 / steps, 4), "numpy_ms_per_iter": round(t_np * 1e3, 1),
                             "device_ms_per_iter": round(hmm / args.iters, 3), "n_iter": n_it, "status": st,
                             "first_elbo_rel_diff_to_numpy": abs(e_dev - float(e1)) / abs(float(e1))})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
