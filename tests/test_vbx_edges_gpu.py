"""GPU checks of the VBx kernels (csrc/vbx.hip) at the sizes where they change their path: the cases of tests/test_vbx_edges_cpu.py, which builds
the inputs and the reference runs and asserts on the CPU that the cases reach the paths they are here for.

A. sdk_vbx and sdk_vbx_hmm (Engine.vbx, Engine.vbx_hmm) for two forced iterations (epsilon = -inf, max_iters = 2) on mixtures laid out in
   speaker runs: gamma, pi and the two ELBO values against the loop-form float64 references (tests/vbx_ref.py, tests/vbx_hmm_ref.py), status 0 and
   n_iter 2.  No decision is compared: with S >> n tens of speaker weights lie at the keep threshold after two iterations, and the kept speakers,
   labels and centroids of such a run say nothing about the kernels.  Tolerance, as tests/test_vbx_hmm_gpu.py takes it: the yardstick of a quantity
   is the larger distance of the float64 reference to its long-double run and to its run with every sum in descending order; the quantity passes
   within 8 x its yardstick + 4 ulp of its largest magnitude.  One case adds the one-ulp run of exp and log to its yardstick
   (test_vbx_edges_cpu.JITTER, with the figures that called for it).
B. sdk_vbx_centroids alone (Engine.vbx_centroids) on constructed responsibilities and speaker weights whose every decision is exact by design: K,
   keep, the labels (one planted tie goes to the lower speaker; a dropped speaker's column holds the maximum of many rows), a kept speaker whose
   column is all zero (the zero centroid), NaN weights, widths above 256 (the second column per thread) and row counts at the 256-row tile's edge;
   cent64 within 8 x the yardstick of vbx_ref.result + 4 ulp, cent its fp32 rounding exactly, rows K.. zero; and no speaker kept at all.
   At d = 320 and 448 the second column is live for one wave and for all waves but one: checked on the CPU (tests/test_vbx_edges_cpu.py prints
   it), without the columns 256.. the reference's centroids move by 0.16, more than 1e13 x the tolerance.
C. sdk_plda_transform alone at d_in = 320 and D0 = 300, where a thread's second column is partial over the input AND over the intermediate
   width, against vbx_ref.transform in float64 within 8 x its distance to the long-double run + 4 ulp.  Checked on the CPU: without the input
   columns 256.. the reference moves by 2.0, without the intermediate ones by 1.8, both more than 1e13 x the tolerance.

Every test prints its figures before it asserts; profiles/vbx_edges_parity.txt records them as measured on an MI355X."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_vbx_edges_cpu as EC  # noqa: E402
import test_vbx_hmm_gpu as HG  # noqa: E402

pytestmark = pytest.mark.gpu
MARGIN, ULPS = HG.MARGIN, HG.ULPS                                         # 8 and 4: the project's rule, unchanged
QUANTITIES = ("gamma", "pi", "elbo")
dev = HG.dev


def entry_name(entry):
    return "sdk_vbx" if entry is None else f"sdk_vbx_hmm P={entry}"


def run_iterations(engine, case, entry):
    """Two forced iterations of one case on the device -> gamma, pi, elbo [2], n_iter, status."""
    n, D, S, _ = case
    m, E, rows, init, _ = HG.mixture(case)
    Ed, rd = dev(E), dev(rows)
    X = engine.plda_transform(Ed, rd, m)
    Phi = m.device_arrays(Ed.device)["Phi"]
    kw = dict(epsilon=-np.inf, max_iters=EC.ITERS)
    out = engine.vbx(X, Phi, dev(init), S, **kw) if entry is None else engine.vbx_hmm(X, Phi, dev(init), S, entry, **kw)
    torch.cuda.synchronize()
    gamma, pi, elbo, n_iter, status = (t.cpu().numpy() for t in out)
    return dict(gamma=gamma, pi=pi, elbo=elbo, n_iter=int(n_iter[0]), status=int(status[0]))


def deviations(got, runs):
    """-> {quantity: (max |d|, yardstick, tolerance, ratio)} of one device run against its reference runs."""
    out = {}
    for q in QUANTITIES:
        want = runs["f64"][q]
        y = HG.yardstick(runs, q)
        tol = MARGIN * y + ULPS * float(np.spacing(np.abs(want).max()))
        ok = got[q].shape == want.shape and bool(np.isfinite(got[q]).all())
        err = float(np.abs(got[q] - want).max()) if ok else np.inf
        out[q] = (err, y, tol, err / y if y > 0 else (0.0 if err == 0 else np.inf))
    return out


# ------------------------------------------------------------------------------------------------ A: the iteration kernels
@pytest.mark.parametrize("S,D", EC.SD, ids=lambda v: str(v))
def test_two_iterations_against_the_float64_reference(engine, S, D):
    worst = {}                                                            # (entry, quantity) -> (ratio, n)
    failed = []
    for case, entry in EC.cases_of(S, D):
        n = case[0]
        runs = EC.edge_runs(case, entry)
        got = run_iterations(engine, case, entry)
        dv = deviations(got, runs)
        print(f"vbx edges S={S} D={D} n={n} {entry_name(entry)}: status {got['status']} n_iter {got['n_iter']}  " +
              "  ".join(f"{q} max|d| {e:.3e} yardstick {y:.3e} tolerance {t:.3e} ratio {r:.2f}" for q, (e, y, t, r) in dv.items()))
        if got["status"] != 0 or got["n_iter"] != EC.ITERS:
            failed.append((n, entry, "status / n_iter"))
        for q, (e, y, t, r) in dv.items():
            if not e <= t:
                failed.append((n, entry, q))
            if r >= worst.get((entry, q), (-1.0, 0))[0]:
                worst[entry, q] = (r, n)
    for entry in EC.ENTRIES:
        print(f"vbx edges S={S} D={D} {entry_name(entry)}: worst ratio " + "  ".join(f"{q} {worst[entry, q][0]:.2f} (n={worst[entry, q][1]})" for q in QUANTITIES))
    assert not failed, failed


@pytest.mark.parametrize("S", [256, 257])
def test_two_runs_of_the_iterations_are_bit_identical(engine, S):
    case = (10, 64, S, 3)
    for entry in EC.ENTRIES:
        a, b = run_iterations(engine, case, entry), run_iterations(engine, case, entry)
        for q in QUANTITIES:
            assert a[q].tobytes() == b[q].tobytes(), (entry, q)
        assert a["n_iter"] == b["n_iter"] == EC.ITERS and a["status"] == b["status"] == 0


# ------------------------------------------------------------------------------------------------ B: the centroids
def run_centroids(engine, c):
    K, keep, labels, cent, cent64 = engine.vbx_centroids(dev(c["gamma"]), dev(c["pi"]), dev(c["E"]), dev(c["rows"]))
    torch.cuda.synchronize()
    return dict(K=int(K.item()), keep=keep.cpu().numpy(), labels=labels.cpu().numpy(), cent=cent.cpu().numpy(), cent64=cent64.cpu().numpy())


@pytest.mark.parametrize("shape", EC.CENTROID_SHAPES, ids=lambda s: "n%d-S%d-d%d" % s)
def test_centroids_on_constructed_inputs(engine, shape):
    n, S, d = shape
    c = EC.centroid_case(shape)
    runs = EC.centroid_runs(shape)
    ref = runs["f64"]
    K = len(ref["keep"])
    if d in EC.PW.WIDTHS:                                                 # asserted on the reference alone, before the device is asked
        EC.centroid_weight(shape)
    got = run_centroids(engine, c)
    again = run_centroids(engine, c)
    want = ref["cent"]
    a = want.astype(np.longdouble)
    y = max(float(np.abs(a - runs[k]["cent"].astype(np.longdouble)).max()) for k in ("ld", "rev"))
    tol = MARGIN * y + ULPS * float(np.spacing(np.abs(want).max()))
    have = got["cent64"][:K]
    err = float(np.abs(have - want).max())
    print(f"vbx edges centroids n={n} S={S} d={d}: K {got['K']} (reference {K})  labels differing {int((got['labels'] != ref['labels']).sum())}  "
          f"cent64 max|d| {err:.3e} yardstick {y:.3e} tolerance {tol:.3e} ratio {err / y if y > 0 else (0.0 if err == 0 else np.inf):.2f}")
    assert got["K"] == K and np.array_equal(got["keep"][:K], ref["keep"]) and (got["keep"][K:] == -1).all()
    assert got["labels"].dtype == np.int32 and np.array_equal(got["labels"], ref["labels"])
    if c["tie"] is not None:
        assert got["labels"][c["tie"][0]] == ref["keep"].tolist().index(c["tie"][1])      # the tie goes to the lower speaker
    assert have.shape == want.shape and np.isfinite(got["cent64"]).all() and err <= tol
    if "zero" in c["roles"]:
        z = ref["keep"].tolist().index(c["roles"].index("zero"))
        assert not got["cent64"][z].any() and not got["cent"][z].any()                    # no weight: the zero centroid
    assert got["cent"].dtype == np.float32 and np.array_equal(got["cent"][:K], got["cent64"][:K].astype(np.float32))
    assert got["cent"].shape == got["cent64"].shape == (S, d) and not got["cent"][K:].any() and not got["cent64"][K:].any()
    for q in ("keep", "labels", "cent", "cent64"):
        assert got[q].tobytes() == again[q].tobytes(), q
    assert got["K"] == again["K"]


def test_centroids_with_no_speaker_kept(engine):
    n, S, d = EC.NONE_KEPT
    got = run_centroids(engine, EC.none_kept_case())
    print(f"vbx edges centroids n={n} S={S} d={d}, every pi <= 1e-12: K {got['K']}")
    assert got["K"] == 0 and (got["keep"] == -1).all() and got["keep"].shape == (S,)
    assert got["labels"].shape == (n,) and (got["labels"] == -1).all()
    assert got["cent"].shape == got["cent64"].shape == (S, d) and not got["cent"].any() and not got["cent64"].any()


# ------------------------------------------------------------------------------------------------ C: the front transform
def test_transform_with_two_partial_second_columns(engine):
    n, d_in, D0, D = EC.TRANSFORM_CASE
    c = EC.transform_case()
    y, tol = EC.transform_tolerance()
    X = engine.plda_transform(dev(c["E"]), dev(c["rows"]), c["m"])
    again = engine.plda_transform(dev(c["E"]), dev(c["rows"]), c["m"])
    torch.cuda.synchronize()
    have = X.cpu().numpy()
    err = float(np.abs(have - c["f64"]).max()) if have.shape == c["f64"].shape else np.inf
    print(f"vbx edges transform n={n} {d_in} -> {D0} -> {D}: max|d| {err:.3e} yardstick {y:.3e} tolerance {tol:.3e} ratio {err / y if y > 0 else np.inf:.2f}")
    assert have.dtype == np.float64 and have.shape == (n, D) and np.isfinite(have).all() and err <= tol
    assert torch.equal(X, again)
