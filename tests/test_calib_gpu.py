"""GPU checks of the calibration pass (sdk_trial_calib, ops_score.trial_calib), of trials.calibrate_scores and of
backend.calibrate_verification / SDK_SCORE_CALIBRATION, against the long-double restatement of tests/calib_ref.py.

Exact inputs.  Entries of A, B and r that are multiples of 2^-6 (tests/test_trials_gpu.py): every score is exact in any order, and
z = a * s + c is bit-equal on host and device because both round the multiplication and the addition separately.  What is left is the error
of a term and of the additions it passes through:

    |device sum - reference sum| <= (C_F + L) * 2^-53 * sum |term|

  L    the additions a term can pass through: its lane's chain, 16 trials per tile and lane over the ceil(tiles / grid) tiles of a workgroup;
       the xor tree over the 64 lanes, 6; the four waves, 3; the workgroups' rows in ascending order, grid.  L = 16 ceil(tiles / grid) + 9 + grid.
  C_F  the error of one term - exp, log1p, two divisions, up to three multiplications, two additions on identical arguments - in units of
       2^-53 of the term.  No documentation of the device math library's ULP bounds ships with the toolchain, so C_F is EIGHT TIMES the worst
       per-term deviation seen in the first GPU run of test_per_term_deviation (WORST_SEEN below, recorded in profiles/ beside the bench
       line).  The test prints the worst ratio of every run.

Rounded inputs.  The device's score lies within delta = (K + 3) u a(i, j) of the long-double product (tests/test_trials_gpu.py's docstring).
loss is 1-Lipschitz in m, w is 1/4-Lipschitz and v is 1/(6 sqrt 3)-Lipschitz, and |dm| = |a| delta, so a sum moves by at most
Lip |a| sum delta; W1, H1 (times s) and H2 (times s^2) also move through their factor s: by the product rule at most
Lip |a| delta |s| + bound(w or v) delta, resp. Lip |a| delta s^2 + bound(v) 2 |s| delta (+ delta^2 terms, below 1e-28 here); S1 by sum delta.
With rounded inputs the two sides also form z = a * s + c from DIFFERENT s, so the two float64 roundings of z are no longer common to both:
each side's z lies within u (|a s| + |z|) of its exact a s + c, which moves m by up to 2 u (|a s| + |z|) more and a sum by Lip times that
(C_F does not hold it: it was measured on bit-equal z).  The bound asserted is the narrower one, without this term; the test also prints
the ratio against the bound that carries it.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calib_ref as CR  # noqa: E402
from conftest import ROOT, sub  # noqa: E402

pytestmark = pytest.mark.gpu

T = sub("trials")
OPS = sub("ops_score")
PLDA = sub("plda")
U53 = 2.0 ** -53
LD = np.longdouble
WORST_SEEN = 3.911                 # units of 2^-53 of a term: the first GPU run's figure (profiles/r31_calib_parity.txt), in H2 at |m| = 24
C_F = 8 * WORST_SEEN
POINTS = [(1.0, 0.0), (0.37, -2.5), (6.0, 40.0)]
SHAPES = [(1, 1, 16, 0), (63, 65, 16, 0), (64, 64, 192, 0), (130, 200, 256, 0), (130, 200, 256, 1), (130, 200, 256, 3), (65, 129, 512, 0)]
assert np.finfo(LD).eps <= 2.0 ** -63, "the reference needs an extended-precision long double"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tensors(A, B, r, la, sa, lb, sb):
    return [dev(A), dev(B), dev(r)] + [dev(np.asarray(x).astype(np.int32)) for x in (la, sa, lb, sb)]


def gpu_sums(engine, d, a, c, max_blocks=0):
    out = OPS.trial_calib(engine, *d, a, c, max_blocks=max_blocks)
    torch.cuda.synchronize()
    return T.sums_to_host(out)


def grid_inputs(N, M, K, seed):
    rng = np.random.default_rng(seed)
    A = rng.integers(-128, 129, (N, K)) / 64.0
    B = rng.integers(-128, 129, (M, K)) / 64.0
    r = rng.integers(-128, 129, M) / 64.0
    la, lb = rng.integers(-1, 5, N), rng.integers(-1, 5, M)
    sa, sb = rng.integers(-1, 4, N), rng.integers(-1, 4, M)
    return A, B, r, la, sa, lb, sb


def additions(N, M, max_blocks):
    """L of the module docstring, from the kernel's reduction."""
    tiles = -(-N // 64) * -(-M // 64)
    grid = min(tiles, 512, max_blocks or tiles)
    return 16 * -(-tiles // grid) + 9 + grid


def worst_ratio(got, ref, L, extra=0.0):
    """max over classes and sums of |got - ref| / bound; counts compared exactly."""
    assert got.n.tolist() == ref["n"] and got.nonfinite.tolist() == ref["nonfinite"] and got.excluded == ref["excluded"]
    err = np.abs(got.sums.astype(LD) - ref["sums"]).astype(np.float64)
    bound = (C_F + L) * U53 * ref["mag"].astype(np.float64) + extra
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


_REF = {}


def exact_case(N, M, K):
    """Inputs, device tensors' sources and the reference sums at the three points, computed once per shape."""
    key = (N, M, K)
    if key not in _REF:
        A, B, r, la, sa, lb, sb = grid_inputs(N, M, K, 100 + N + K)
        if N == 1:
            la[:], lb[:], sa[:], sb[:] = 2, 2, 0, 1
        S, cls = A @ B.T + r[None, :], CR.classes(la, sa, lb, sb)                     # exact in float64
        _REF[key] = ((A, B, r, la, sa, lb, sb), S, cls, {p: CR.sums(S, cls, *p) for p in POINTS})
    return _REF[key]


# ---- the per-term error, measured ----------------------------------------------------------------------------------------------------------
def test_per_term_deviation(engine):
    """One trial per launch (N = M = 1): the sums ARE the terms.  Scores through r alone, 2^-6 apart, so that m covers +-60 at every point."""
    A, B = np.zeros((1, 16)), np.zeros((1, 16))
    worst, where = 0.0, None
    for a, c in POINTS:
        for m in np.linspace(-60.0, 60.0, 41):
            s = float(np.round((m - c) / a * 64.0) / 64.0)
            for same in (0, 1):
                d = tensors(A, B, np.asarray([s]), [1], [-1], [1 if same else 2], [-1])
                got, ref = gpu_sums(engine, d, a, c), CR.sums(np.asarray([s]), np.asarray([same]), a, c)
                assert got.n.tolist() == ref["n"] and got.n[same] == 1
                mag = ref["mag"][same].astype(np.float64)
                dev_ = np.abs(got.sums[same].astype(LD) - ref["sums"][same]).astype(np.float64)
                assert (dev_[mag == 0] == 0).all()
                ratio = float((dev_[mag > 0] / (U53 * mag[mag > 0])).max())
                if ratio > worst:
                    worst, where = ratio, (a, c, s, same, CR.NAMES[int(np.argmax(np.where(mag > 0, dev_ / np.maximum(mag, 1e-300), 0)))])
    print(f"calibration per-term deviation: worst {worst:.3f} x 2^-53 of the term at {where}; C_F = {C_F}")
    assert worst <= C_F                                          # a later run above the first one's figure is worth a look; above C_F the bound is void


# ---- exact inputs --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,K,max_blocks", SHAPES)
def test_sums_on_exact_inputs(engine, N, M, K, max_blocks):
    inputs, S, cls, refs = exact_case(N, M, K)
    d = tensors(*inputs)
    L = additions(N, M, max_blocks)
    for (a, c), ref in refs.items():
        got = gpu_sums(engine, d, a, c, max_blocks)
        ratio = worst_ratio(got, ref, L)
        print(f"calib sums N={N} M={M} K={K} max_blocks={max_blocks} (a, c)=({a}, {c}): n {got.n.tolist()}, L {L}, worst |err| / bound {ratio:.4f}")
        assert ratio <= 1.0
        assert int(got.n.sum()) + int(got.nonfinite.sum()) + got.excluded == N * M


def test_edges_on_exact_inputs(engine):
    # a tile whose trials are all excluded (rows 64 .. 127 have no label), inside a matrix of 3 x 2 tiles
    A, B, r, la, sa, lb, sb = grid_inputs(150, 100, 32, 9)
    la[64:128] = -1
    S, cls = A @ B.T + r[None, :], CR.classes(la, sa, lb, sb)
    got = gpu_sums(engine, tensors(A, B, r, la, sa, lb, sb), 0.37, -2.5)
    assert worst_ratio(got, CR.sums(S, cls, 0.37, -2.5), additions(150, 100, 0)) <= 1.0 and got.excluded >= 64 * 100
    # a class with no trial: no model label equals a test label
    got = gpu_sums(engine, tensors(A, B, r, np.abs(la), sa, np.abs(lb) + 10, sb), 1.0, 0.0)
    assert got.n[1] == 0 and not got.sums[1].any() and got.n[0] > 0
    assert worst_ratio(got, CR.sums(S, CR.classes(np.abs(la), sa, np.abs(lb) + 10, sb), 1.0, 0.0), additions(150, 100, 0)) <= 1.0
    # +inf, -inf and NaN through r: counted, and left out of every sum
    r2 = r.copy()
    r2[[3, 70, 99]] = [np.inf, -np.inf, np.nan]
    S2 = S.copy()
    S2[:, [3, 70, 99]] = [np.inf, -np.inf, np.nan]
    got, ref = gpu_sums(engine, tensors(A, B, r2, la, sa, lb, sb), 6.0, 40.0), CR.sums(S2, cls, 6.0, 40.0)
    assert worst_ratio(got, ref, additions(150, 100, 0)) <= 1.0 and int(got.nonfinite.sum()) == int((cls[:, [3, 70, 99]] >= 0).sum()) > 0
    assert np.isfinite(got.sums).all()


def test_two_runs_are_equal_bit_for_bit_and_grids_agree_to_rounding(engine):
    A, B, r, la, sa, lb, sb = grid_inputs(300, 260, 64, 7)
    A, B = A + 1e-3 * np.random.default_rng(1).standard_normal(A.shape), B * (1 + 2.0 ** -30)       # rounded inputs
    d = tensors(A, B, r, la, sa, lb, sb)
    one, two, single = gpu_sums(engine, d, 0.37, -2.5), gpu_sums(engine, d, 0.37, -2.5), gpu_sums(engine, d, 0.37, -2.5, max_blocks=1)
    assert np.array_equal(one.sums.view(np.int64), two.sums.view(np.int64)) and one.n.tolist() == two.n.tolist() == single.n.tolist()
    assert one.excluded == single.excluded and one.nonfinite.tolist() == single.nonfinite.tolist()
    # both lie within their bound of the exact sum of the device's own terms, so within the sum of the bounds of each other
    mag = CR.sums(CR.scores(A, B, r), CR.classes(la, sa, lb, sb), 0.37, -2.5)["mag"].astype(np.float64)
    bound = (additions(300, 260, 0) + additions(300, 260, 1)) * U53 * mag * (1 + 1e-6)
    assert (np.abs(one.sums - single.sums) <= bound).all()


# ---- rounded inputs ------------------------------------------------------------------------------------------------------------------------
def test_unit_rows_within_the_lipschitz_bound(engine):
    rng = np.random.default_rng(11)
    N, M, K, nspk = 150, 170, 192, 6
    centres = rng.standard_normal((nspk, K))
    la, lb = rng.integers(0, nspk, N), rng.integers(0, nspk, M)
    unit = lambda X: (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)        # noqa: E731
    A, B = unit(centres[la] + 1.5 * rng.standard_normal((N, K))), unit(centres[lb] + 1.5 * rng.standard_normal((M, K)))
    sa, sb = rng.integers(-1, 5, N), rng.integers(-1, 5, M)
    r = np.zeros(M)
    S, cls = CR.scores(A, B, r), CR.classes(la, sa, lb, sb)
    delta = (K + 3) * U53 * (np.abs(A) @ np.abs(B).T + np.abs(r)[None, :]) * (1 + 2.0 ** -40)
    d = tensors(A, B, r, la, sa, lb, sb)
    lip = np.asarray([1.0, 0.25, 0.25, 1 / (6 * math.sqrt(3)), 1 / (6 * math.sqrt(3)), 1 / (6 * math.sqrt(3)), 0.0])
    top = np.asarray([0.0, 0.0, 1.0, 0.0, 0.25, 0.25, 1.0])          # the bound of the factor that multiplies s (w <= 1, v <= 1/4; S1: 1)
    power = np.asarray([0, 0, 1, 0, 1, 2, 1])

    def zround(a, c):
        """The module docstring's last term: Lip * 2 u (|a s| + |z|) per trial, times |s| or s^2 where the term carries them."""
        out = np.zeros((2, 7))
        for k in (0, 1):
            sk = np.abs(S[cls == k])
            dm = 2 * U53 * (abs(a) * sk + np.abs(a * S[cls == k] + c)) * (1 + 1e-9)
            for t in range(7):
                out[k, t] = (lip[t] * dm * sk ** power[t]).sum()
        return out

    for a, c in ((1.0, 0.0), (14.0, -3.0)):
        got, ref = gpu_sums(engine, d, a, c), CR.sums(S, cls, a, c)
        extra = np.zeros((2, 7))
        for k in (0, 1):
            dk, sk = delta[cls == k], np.abs(S[cls == k])
            for t in range(7):
                moved = lip[t] * abs(a) * dk * sk ** power[t]
                if power[t]:
                    moved = moved + top[t] * power[t] * sk ** (power[t] - 1) * dk
                extra[k, t] = moved.sum() * (1 + 1e-9)
        ratio = worst_ratio(got, ref, additions(N, M, 0), extra)
        full = worst_ratio(got, ref, additions(N, M, 0), extra + zround(a, c))
        print(f"calib unit rows (a, c)=({a}, {c}): worst |err| / bound {ratio:.4f} (with the roundings of z in the bound: {full:.4f})")
        assert ratio <= 1.0                                      # the narrower of the two bounds is the one asserted


# ---- the fit -------------------------------------------------------------------------------------------------------------------------------
def speaker_grid_inputs(N=130, M=150, K=64, nspk=5, seed=31):
    """Exact inputs whose target scores lie above the nontarget ones on average and overlap with them."""
    rng = np.random.default_rng(seed)
    centres = rng.integers(-24, 25, (nspk, K)) / 64.0
    la, lb = rng.integers(0, nspk, N), rng.integers(0, nspk, M)
    A = centres[la] + rng.integers(-48, 49, (N, K)) / 64.0
    B = centres[lb] + rng.integers(-48, 49, (M, K)) / 64.0
    return A, B, rng.integers(-16, 17, M) / 64.0, la, rng.integers(-1, 6, N), lb, rng.integers(-1, 6, M)


def test_calibrate_scores_agrees_with_the_host_driver_on_reference_sums(engine):
    A, B, r, la, sa, lb, sb = speaker_grid_inputs()
    S, cls = A @ B.T + r[None, :], CR.classes(la, sa, lb, sb)
    lo, hi = -64.0, 64.0
    got = T.calibrate_scores(engine, *tensors(A, B, r, la, sa, lb, sb), "plda", (lo, hi))

    def ref_sums(a, c):
        res = CR.sums(S, cls, a, c)
        return T.CalibSums(np.asarray(res["n"]), res["sums"].astype(np.float64), np.asarray(res["nonfinite"]), res["excluded"])

    want = T.calibration_from_passes(T.trial_hist_host(A, B, r, la, sa, lb, sb, lo, hi), lambda b: T.trial_hist_host(A, B, r, la, sa, lb, sb, lo, hi, 0, 4096 * b),
                                     ref_sums, "plda", lo, hi)
    assert got.converged and want.converged and got.a > 0
    assert (got.n_target, got.n_nontarget, got.n_nonfinite, got.n_excluded) == (want.n_target, want.n_nontarget, 0, want.n_excluded)
    prior, theta = got.prior, math.log(got.prior / (1 - got.prior))
    at = CR.sums(S, cls, want.a, want.b + theta)
    J, _, H = (np.asarray(x, np.float64) for x in CR.objective(at, prior))
    B_sum = (C_F + additions(130, 150, 0)) * U53 * at["mag"].astype(np.float64)             # the bound of every device sum at the solution
    u0, u1 = (1 - prior) / at["n"][0], prior / at["n"][1]
    grad_bound = max(u0 * B_sum[0][2] + u1 * B_sum[1][2], u0 * B_sum[0][1] + u1 * B_sum[1][1])
    tol = float(np.linalg.norm(np.linalg.inv(H), 2) * (grad_bound + 1e-10 * J))
    dist = max(abs(got.a - want.a), abs(got.b - want.b))
    print(f"calibrate_scores: a {got.a:.6f} b {got.b:.6f} in {got.n_passes} passes, |device - host| {dist:.3e} of {tol:.3e}; cllr {got.cllr_raw:.4f} -> "
          f"{got.cllr:.4f} (coarse minimum {got.min_cllr_coarse:.4f}), act_dcf {got.act_dcf:.4f}, min_dcf {got.min_dcf:.4f}")
    assert dist <= tol
    q = T.threshold_q(got.bayes_threshold, lo, hi)
    assert got.act_dcf == CR.dcf_at(S, cls, lo, hi, q, 0.01, 1.0, 1.0) and got.min_dcf == want.min_dcf
    assert got.min_cllr_coarse == want.min_cllr_coarse and abs(got.min_cllr_coarse - float(CR.pav_min_cllr(*pav_cells(S, cls, lo, hi)))) <= 1e-13
    for name, (a, c) in (("cllr_raw", (1.0, 0.0)), ("cllr", (got.a, got.b))):
        res = CR.sums(S, cls, a, c)
        bound = float(((C_F + additions(130, 150, 0)) * U53 * res["mag"][:, 0].astype(np.float64) / np.asarray(res["n"])).sum() / (2 * math.log(2)))
        assert abs(getattr(got, name) - float(CR.cllr(res))) <= bound * (1 + 1e-6) + 4 * U53
    assert got.cllr <= got.cllr_raw


def pav_cells(S, cls, lo, hi):
    q, nan = CR.quantise(S, lo, hi)
    cell = np.where(q < 0, 0, np.where(q >= 2 ** 24, 4097, 1 + (q >> 12)))
    live = (cls >= 0) & ~nan
    return (np.bincount(cell[live & (cls == 1)], minlength=4098), np.bincount(cell[live & (cls == 0)], minlength=4098))


# ---- argument errors -----------------------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    A, B, r, la, sa, lb, sb = grid_inputs(8, 8, 32, 6)
    d = tensors(A, B, r, la, sa, lb, sb)
    sums, counts = torch.zeros(14, dtype=torch.float64, device="cuda"), torch.zeros(5, dtype=torch.int64, device="cuda")
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    lib, ctx = engine.lib, engine.ctx

    def raw(K=32, N=8, M=8, a=1.0, c=0.0, max_blocks=0, A_=d[0].data_ptr(), ws_=ws.data_ptr(), ws_bytes=4096):
        return lib.sdk_trial_calib(ctx, A_, N, d[1].data_ptr(), d[2].data_ptr(), M, K, d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(),
                                   a, c, max_blocks, sums.data_ptr(), counts.data_ptr(), ws_, ws_bytes, None)

    assert raw() == 0
    for kw in (dict(K=24), dict(K=528), dict(K=0), dict(N=0), dict(M=(1 << 20) + 1), dict(A_=None), dict(A_=d[0].data_ptr() + 8), dict(a=float("nan")),
               dict(a=float("inf")), dict(c=float("-inf")), dict(c=float("nan")), dict(max_blocks=-1), dict(ws_=None), dict(ws_bytes=64),
               dict(ws_=ws.data_ptr() + 8)):
        assert raw(**kw) == 2, kw
        assert b"sdk_trial_calib" in lib.sdk_last_error()
    assert lib.sdk_trial_calib_workspace_bytes(0, 8, 0) == 0 and b"sdk_trial_calib_workspace_bytes" in lib.sdk_last_error()
    assert lib.sdk_trial_calib_workspace_bytes(8, 8, 0) == 256 and lib.sdk_trial_calib_workspace_bytes(1 << 20, 1 << 20, 0) == 512 * 128
    torch.cuda.synchronize()
    odd = torch.zeros((8, 24), dtype=torch.float64, device="cuda")
    for call in (lambda: OPS.trial_calib(engine, odd, odd, *d[2:], 1.0, 0.0), lambda: OPS.trial_calib(engine, *d, float("nan"), 0.0),
                 lambda: OPS.trial_calib(engine, *d, 1.0, float("inf")), lambda: OPS.trial_calib(engine, d[0].float(), *d[1:], 1.0, 0.0),
                 lambda: OPS.trial_calib(engine, d[0].cpu(), *d[1:], 1.0, 0.0), lambda: OPS.trial_calib(engine, *d, 1.0, 0.0, max_blocks=-1)):
        with pytest.raises(ValueError):
            call()


# ---- the Backend ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cosine", "plda"])
def test_backend_calibrate_and_apply(tmp_path, monkeypatch, kind):
    sys.path.insert(0, str(ROOT / "evals"))
    from run_eval import render_voice
    wav, BK = sub("wav"), sub("backend")
    monkeypatch.setenv("SPEAKERS_EMBEDDINGS_DIR", str(tmp_path / "store"))
    monkeypatch.setenv("SDK_CACHE_DIR", str(tmp_path / "cache"))
    for v in ("SDK_COHORT", "SDK_COHORT_THRESHOLD", "SDK_NO_TORCH", "SDK_SCORE_PLDA_DIM", "SDK_SCORE_PLDA_THRESHOLD", "SDK_SCORE_PLDA_COUNT",
              "SDK_SCORE_PLDA_TRANSFORM", "SDK_SCORE_PLDA", "SDK_SCORE_CALIBRATION", "SDK_SCORE_PRIOR"):
        monkeypatch.delenv(v, raising=False)
    if kind == "plda":
        tnpz, pnpz = tmp_path / "xvec_transform.npz", tmp_path / "plda.npz"
        monkeypatch.setenv("SDK_SCORE_PLDA_TRANSFORM", str(tnpz))
        monkeypatch.setenv("SDK_SCORE_PLDA", str(pnpz))
        monkeypatch.setenv("SDK_SCORE_PLDA_THRESHOLD", "-1e9")          # every window votes: rows to compare
    be = BK.Backend()
    if kind == "plda":
        PLDA.save_plda(PLDA.synthetic_plda(be.embedding_dim, 128), tnpz, pnpz)

    def recording(name, tag, seconds, seed):
        path = tmp_path / f"{name}.wav"
        wav.write_wav_s16(path, render_voice(tag, seconds, seed))
        return path

    profiles = []
    for i, (sid, takes) in enumerate((("ann", 2), ("bob", 1), ("cy", 1))):
        embs = []
        for t in range(takes):
            rec = be.enroll_speaker(recording(f"enroll_{sid}_{t}", sid, 5.0, 100 + 7 * i + 50 * t))
            embs.append({"id": f"emb-{sid}-{t}", "external_id": rec["external_id"], "model_version": rec["model_version"], "trust_level": "high"})
        profiles.append({"id": sid, "names": {"default": sid.title()}, "embeddings": {"mi355x": embs}})
    # two recordings carry the other speaker's id: the classes overlap whatever the (synthetic) network separates, so the fit has a minimiser
    voices = ("ann", "bob", "cy", "stranger", "bob", "ann")
    ids = ["ann", "bob", "cy", "nobody-enrolled", "ann", "bob"]
    paths = [recording(f"dev_{j}", tag, 4.0, 300 + j) for j, tag in enumerate(voices)]
    out = tmp_path / "calibration.json"
    cal = BK.calibrate_verification(be, paths, ids, profiles, out_path=out)
    assert cal.converged and cal.kind == kind and cal.a > 0 and out.exists() and T.load_calibration(out) == cal
    res = be.score_verification(paths, ids, profiles)
    assert (cal.n_target, cal.n_nontarget, cal.n_excluded) == (res.n_target, res.n_nontarget, res.n_excluded) and cal.min_dcf == res.min_dcf
    assert cal.cllr <= cal.cllr_raw and cal.min_dcf <= cal.act_dcf
    print(f"calibrate_verification {kind}: a {cal.a:.4f} b {cal.b:.4f}, cllr {cal.cllr_raw:.4f} -> {cal.cllr:.4f}, {cal.n_passes} passes")
    plain = be.identify_speaker(paths[0], profiles, threshold=-1.0)
    plain_verify = be.verify_speaker(paths[0], profiles[0], threshold=-1.0)
    monkeypatch.setenv("SDK_SCORE_CALIBRATION", str(out))
    monkeypatch.setenv("SDK_SCORE_PRIOR", "0.1")
    be2 = BK.Backend()
    rows = be2.identify_speaker(paths[0], profiles, threshold=-1.0)
    key = "similarity" if kind == "cosine" else "llr"
    assert len(rows) == len(plain) > 0
    for w, g in zip(plain, rows):
        assert {k: g[k] for k in w} == w and list(g)[:len(w)] == list(w) and set(g) - set(w) == {"calibrated_llr", "posterior"}
        llr = float(np.float64(cal.a) * np.float64(w[key]) + np.float64(cal.b))
        assert g["calibrated_llr"] == llr and abs(g["posterior"] - 1 / (1 + math.exp(-(llr + math.log(0.1 / 0.9))))) <= 1e-15
    assert be2.identify_many([paths[0], paths[1]], profiles, threshold=-1.0)[0] == rows
    got_verify = be2.verify_speaker(paths[0], profiles[0], threshold=-1.0)
    assert {k: got_verify[k] for k in plain_verify} == plain_verify and set(got_verify) - set(plain_verify) == {"calibrated_llr", "posterior"}
    monkeypatch.setenv("SDK_COHORT", str(tmp_path / "cohort.npy"))
    monkeypatch.setenv("SDK_COHORT_THRESHOLD", "1.0")
    for v in ("SDK_SCORE_PLDA_TRANSFORM", "SDK_SCORE_PLDA", "SDK_SCORE_CALIBRATION"):
        monkeypatch.delenv(v, raising=False)
    with pytest.raises(ValueError, match="AS-norm trials are not built"):
        BK.calibrate_verification(BK.Backend(), paths, ids, profiles)
