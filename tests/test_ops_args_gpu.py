"""GPU checks of the refusal paths that moved to _args.py, for the entry points without a refusal test of their own: plda_fit_stats,
plda_project, the ws= of cohort_stats and plda_score_topk, stream_reset, stream_step, stream_flush, the diarize_ops wrappers
(powerset_decode, diarize_masks, diarize_reconstruct, diarize_centroids' rows and labels, the grouped assign, fold and reconstruct,
diarize_first_seen, diarize_renumber), ResNet34.forward_masked and score.score_tables.
Per entry point: a valid call (a shape an existing GPU test of it runs), every single-fault refusal of every tensor argument - wrong
dtype, one wrong extent, a strided view, a host tensor - and the valid call again, bit for bit the first.  A refusal is a ValueError raised
by Python before the library is reached: while the refusals run, the engine's library is replaced by one that fails the test on any call
but a sizer, so a check that lets a bad argument through fails here and never hands it to a kernel."""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plda_fit_ref as FR  # noqa: E402
import stream_ref as SR  # noqa: E402
import test_der_gpu as TD  # noqa: E402
import test_diarize_gpu as TG  # noqa: E402
import test_diarize_many_cpu as MC  # noqa: E402
import test_plda_score_gpu as TP  # noqa: E402

PKG = "speaker-diarization-toolkit_amd"
P = importlib.import_module(f"{PKG}.plda")
dz = importlib.import_module(f"{PKG}.diarize")
seg = importlib.import_module(f"{PKG}.segmentation")
rn = importlib.import_module(f"{PKG}.resnet")
sc = importlib.import_module(f"{PKG}.score")
A = importlib.import_module(f"{PKG}._args")
LIB = importlib.import_module(f"{PKG}._lib")
pytestmark = pytest.mark.gpu

OTHER_DTYPE = {torch.float32: torch.float16, torch.float64: torch.float32, torch.int32: torch.int64, torch.int64: torch.int32, torch.uint8: torch.int8}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class NoLaunch:
    """The engine's library while refusals run: a sizer or the error text passes through, anything else fails the test where it is asked for."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name.endswith("_workspace_bytes") or name in ("sdk_last_error", "sdk_resnet_last_map_frames"):      # host arithmetic: sizes and the error text
            return getattr(self._lib, name)
        raise AssertionError(f"{name} was reached: the refusal must come before any library call")


def faults(t, extent=None):
    """The four single-fault variants of a valid tensor argument (extent: how to get one wrong extent; default: the last one, shortened)."""
    assert t.is_contiguous() and t.shape[-1] >= 2
    return {"dtype": t.to(OTHER_DTYPE[t.dtype]),
            "extent": (extent or (lambda x: x[..., :-1].contiguous()))(t),
            "strided": t.repeat_interleave(2, dim=-1)[..., ::2],
            "host": t.cpu()}


def bits(out):
    out = out if isinstance(out, (tuple, list)) else (out,)
    return [t.detach().clone().contiguous().view(torch.uint8).cpu() for t in out if t is not None]


def exercise(engine, monkeypatch, call, args: dict, extents: dict = {}, prepare=lambda: None, strided_ok=()):
    """call(prepare(), **args) is the valid call (prepare: what it needs from the library beforehand, such as a fresh stream state); every
    tensor in args is then replaced by each of its faults in turn.  strided_ok: the arguments the wrapper makes contiguous itself - their
    strided view is no fault and must give the valid call's result."""
    first = bits(call(prepare(), **args))
    torch.cuda.synchronize()
    ctx, tried, views = prepare(), 0, {}
    with monkeypatch.context() as m:
        m.setattr(engine, "lib", NoLaunch(engine.lib))
        for name, t in args.items():
            for kind, bad in faults(t, extents.get(name)).items():
                if kind == "strided":
                    assert bad.shape == t.shape and not bad.is_contiguous() and bits(bad.contiguous())[0].equal(bits(t)[0])
                    if name in strided_ok:
                        views[name] = bad
                        continue
                with pytest.raises(ValueError) as ei:
                    call(ctx, **{**args, name: bad})
                assert not isinstance(ei.value, LIB.SdkError), (name, kind)
                print(f"  {name} ({kind}): {ei.value}")
                tried += 1
    assert tried == 4 * len(args) - len(views) and sorted(views) == sorted(strided_ok)
    for label, a in [(f"with a strided {name}", {**args, name: view}) for name, view in views.items()] + [("after the refusals", args)]:
        again = bits(call(prepare(), **a))
        torch.cuda.synchronize()
        assert len(first) == len(again) and all(torch.equal(x, y) for x, y in zip(first, again)), f"the valid call {label} differs"


def test_plda_fit_stats(engine, monkeypatch):
    E, lab, _ = FR.labelled_rows(2 + 64, 2, 64, 1)                              # test_plda_fit_gpu's case (N, d, K) = (2, 64, 1)
    args = dict(rows=dev(E), labels=dev(lab), mean1=dev(E.astype(np.float64).mean(0)))

    def call(_, rows, labels, mean1):
        out = engine.plda_fit_stats(rows, labels, 1, mean1=mean1)
        return [out[q] for q in ("counts", "sums", "total", "scatter", "status")]
    exercise(engine, monkeypatch, call, args)


def test_plda_project(engine, monkeypatch):
    N, d_in, D0 = 1, 64, 64                                                     # test_plda_fit_gpu's smallest projection
    E, _, _ = FR.labelled_rows(N + D0, N, d_in, 1)
    m = P.synthetic_plda(d_in, D0, seed=N, lda_dim=64)
    exercise(engine, monkeypatch, lambda _, **a: engine.plda_project(**a), dict(E=dev(E), mean1=dev(m.mean1), lda=dev(m.lda), mean2=dev(m.mean2)))


def test_workspace_arguments(engine, monkeypatch):
    """ws=: a contiguous uint8 device tensor of any length (a short one is the library's refusal, tested with the kernels)."""
    rank = {"ws": lambda t: t.reshape(-1, 1)}                                    # any length is a valid extent: the wrong shape is a second dimension
    c = TP.case(70, 100, 1, 128)                                                 # test_plda_score_gpu's refusal case
    X, G, r = dev(c["X"]), dev(c["G"]), dev(c["r"])
    need = engine.lib.sdk_plda_score_workspace_bytes(70, 100, 1)
    exercise(engine, monkeypatch, lambda _, ws: engine.plda_score_topk(X, G, r, ws=ws), dict(ws=torch.zeros(need, dtype=torch.uint8, device="cuda")), rank)
    rng = np.random.default_rng(31)                                              # test_snorm_gpu's refusal case: 6 rows, a cohort of 50, d = 192, K = 10

    def unit(a):
        return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    E, Cn = dev(unit(rng.standard_normal((6, 192)))), dev(unit(rng.standard_normal((50, 192))))
    need = engine.lib.sdk_cohort_stats_workspace_bytes(6, 50, 10)
    exercise(engine, monkeypatch, lambda _, ws: engine.cohort_stats(E, Cn, 10, ws=ws), dict(ws=torch.zeros(need, dtype=torch.uint8, device="cuda")), rank)


def test_stream_calls(engine, monkeypatch):
    """A bank of three streams on one generated chunk, as test_stream_gpu's inactive-stream check feeds it."""
    hop = latency = 8000
    s = SR.make_stream(300 % 97, 64, 300, hop, n_speakers=3)
    R, d = 3, 64
    step_args = dict(E=dev(np.tile(s["E"][0], (R, 1))), info=dev(np.tile(s["info"][0], (R, 1, 1))), cls=dev(np.tile(s["cls"][0], (R, 1))),
                     starts=torch.zeros(R, dtype=torch.int64, device="cuda"), active=torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda"))
    flush_args = dict(n_samples=torch.full((R,), 300, dtype=torch.int64, device="cuda"), active=step_args["active"])

    def rows(st):
        return [st.buf, st.labels, st.score, st.K, st.emit_lo, st.emit_n, st.count, st.speakers]

    def fresh():
        return engine.stream_state(R, 4, d)

    def stepped():
        return engine.stream_step(fresh(), *step_args.values(), hop, latency, 0.6)

    def reset(st, which):
        engine.stream_reset(st, which)
        return rows(st)
    exercise(engine, monkeypatch, lambda st, **a: rows(engine.stream_step(st, *a.values(), hop, latency, 0.6)), step_args,
             {"cls": lambda t: t[:-1]}, prepare=fresh)                           # cls is [R, F] for any F: the wrong extent is R
    exercise(engine, monkeypatch, lambda st, **a: rows(engine.stream_flush(st, *a.values())), flush_args, prepare=stepped)
    exercise(engine, monkeypatch, reset, dict(which=torch.tensor([0, 0, 1], dtype=torch.uint8, device="cuda")), prepare=stepped)


def test_first_seen_and_renumber(engine, monkeypatch):
    """test_diarize_many_gpu's renumbering case: four recordings, their speakers tables and cluster counts."""
    tabs, frame_off, cent_off = MC.speakers_case(2)
    K = int(cent_off[-1])
    rng = np.random.default_rng(0)
    chunk_off = MC.offsets([9, 4, 3, 20])
    labels = np.concatenate([rng.integers(-1, max(k, 1), (c, 3)) if k else np.full((c, 3), -1) for c, k in zip(np.diff(chunk_off), np.diff(cent_off))]).astype(np.int32)
    n = np.array([0 if g == 0 else 495 + 270 * (g - 1) + 1 for g in np.diff(frame_off)], np.int64)
    tab = dz.GroupTables(engine, chunk_off, frame_off, n).set_clusters(cent_off)
    exercise(engine, monkeypatch, lambda _, speakers: dz.diarize_first_seen(engine, speakers, tab), dict(speakers=dev(np.concatenate(tabs))))
    first = dz.diarize_first_seen(engine, dev(np.concatenate(tabs)), tab)

    def renumber(_, first, labels, cent, cent64):
        labels = labels.clone() if labels.is_cuda and labels.is_contiguous() else labels        # the valid call rewrites its labels in place
        return list(dz.diarize_renumber(engine, first, labels, cent, cent64, tab)) + [labels]
    exercise(engine, monkeypatch, renumber, dict(first=first, labels=dev(labels), cent=dev(rng.standard_normal((K, 64)).astype(np.float32)),
                                                  cent64=dev(rng.standard_normal((K, 64)))))


def test_decode_masks_and_reconstruct(engine, monkeypatch):
    """test_diarize_gpu's shapes: one chunk of logp, nine class tables at T4 = 1, the 21.4-s recording at a 0.5-s step with K = 1."""
    rng = np.random.default_rng(0)
    logp = dev(rng.standard_normal((1, TG.F, 7)).astype(np.float32))
    assert A.tensor("test", "logp", logp, "float32", (1, None, 7)) is logp                      # the checker returns what it took
    exercise(engine, monkeypatch, lambda _, logp: dz.powerset_decode(engine, logp), dict(logp=logp), strided_ok=("logp",))
    row = {"cls": lambda t: t[0]}                                                # [C, F] for any C and F: the wrong shape is one dimension
    exercise(engine, monkeypatch, lambda _, cls: dz.diarize_masks(engine, cls, 1), dict(cls=dev(TG.random_cls(rng, 9))), row)
    n = int(21.4 * 16000) + 131
    st = seg.chunk_starts(n, 0.5)
    rng = np.random.default_rng(214 + 1)
    args = dict(cls=dev(TG.random_cls(rng, len(st))), starts=dev(st.astype(np.int32)), labels=dev(rng.integers(-1, 1, (len(st), 3)).astype(np.int32)))
    exercise(engine, monkeypatch, lambda _, **a: dz.diarize_reconstruct(engine, a["cls"], a["starts"], a["labels"], 1, n, None, want_act=True), args, row,
             strided_ok=("starts", "labels"))


def test_grouped_wrappers(engine, monkeypatch):
    """test_diarize_many_gpu's cases: the reconstruction of five recordings at a 1-s step, the assignment at d = 64, the fold of five."""
    n, starts, cls, labels, chunk_off, frame_off, cent_off = MC.reconstruct_case(1.0, [3, 0, 1, 70, 3], 17)
    tab = dz.GroupTables(engine, chunk_off, frame_off, n, np.concatenate(starts)).set_clusters(cent_off, want_act=True)
    exercise(engine, monkeypatch, lambda _, cls, labels: dz.diarize_reconstruct_grouped(engine, cls, labels, tab, None, want_act=True),
             dict(cls=dev(cls), labels=dev(labels)), {"cls": lambda t: t[:-1]})  # cls is [C, F] for any F: the wrong extent is C
    E, info, cent, chunk_off, cent_off, _ = MC.assign_cases(64, 3)
    tab = dz.GroupTables(engine, chunk_off, np.zeros_like(chunk_off), np.zeros(len(chunk_off) - 1, np.int64)).set_clusters(cent_off)
    exercise(engine, monkeypatch, lambda _, E, info, cent: dz.diarize_assign_grouped(engine, E, info, cent, tab, True),
             dict(E=dev(E), info=dev(info), cent=dev(np.concatenate([cent, np.zeros((1, 64))]))))
    cases = MC.fold_cases(5)
    _, sizes, cl_off, eff, cent_off, _, _ = MC.fold_tables(cases)
    E = np.concatenate([c[0] for c in cases]).astype(np.float32)
    cut = np.concatenate([c[1].astype(np.int64) + int(cl_off[r]) for r, c in enumerate(cases)]).astype(np.int32)
    rows = np.arange(len(cut), dtype=np.int32)
    line = {"rows": lambda t: t.reshape(-1, 1), "cut": lambda t: t.reshape(-1, 1)}      # [n] for any n: the wrong shape is a second dimension
    exercise(engine, monkeypatch, lambda _, rows, labels: dz.diarize_centroids(engine, dev(E), rows, labels, int(cl_off[-1])),
             dict(rows=dev(rows), labels=dev(cut)), line, strided_ok=("rows", "labels"))
    _, c64 = dz.diarize_centroids(engine, dev(E), dev(rows), dev(cut), int(cl_off[-1]))
    exercise(engine, monkeypatch, lambda _, cent, cut: dz.diarize_fold_grouped(engine, cent, sizes, cl_off, eff, cent_off, cut), dict(cent=c64, cut=dev(cut)), line)


def test_resnet_forward_masked(engine, monkeypatch):
    """test_diarize_gpu's masked forward: two 10-s chunks, three weight rows each."""
    B, S = 2, 3
    net = rn.ResNet34(engine, rn.synthetic_weights(0), precision=0)
    feats, _ = TG.chunk_feats(engine, 0, B, 9)
    rng = np.random.default_rng(2)
    args = dict(w=dev(rng.random((B, S, TG.T4_CHUNK)).astype(np.float32)), valid=torch.tensor([[1, 1, 1], [1, 0, 1]], dtype=torch.int32, device="cuda"))
    exercise(engine, monkeypatch, lambda _, w, valid: net.forward_masked(feats, B, TG.T_CHUNK, w, valid), args)


def test_score_tables(engine, monkeypatch):
    """test_der_gpu's pack 0: seven recordings, their speakers tables on the packed grid."""
    refs, hyps = TD.pack_case(0)
    tab = TD.tables(engine, TD.N_SAMPLES, TD.K_SETS[0])
    ref = sc.rasterise_references(engine, tab, refs, 0.0, False)

    def call(_, speakers):
        t = sc.score_tables(engine, speakers, tab, ref)
        return t.tally, t.correct, t.mapping, t.co
    exercise(engine, monkeypatch, call, dict(speakers=dev(np.concatenate(hyps))))
