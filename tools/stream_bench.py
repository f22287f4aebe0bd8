"""Streaming diarization (stream.py, csrc/stream.hip) on one MI355X -> one JSON line.

For R = 1 / 16 / 64 / 256 live streams of generated audio at step_s = 0.5: the device time of sdk_stream_step alone - a window of WINDOW
back-to-back launches between two HIP events, on the embeddings of a real bank step, every launch one hop further on, divided by WINDOW;
the host's time to submit them is recorded beside it (submit_us: where it is the larger, the window measures the submission, not the
kernel) and so is one event-timed wrapper call (step_call_ms: it includes the submission gap and the event floor) - the time of a whole
bank step split into segmentation, embedding (decode, masks, fbank, ResNet34, L2 norm),
the step kernel and the host's share (tables up, the one download, bookkeeping; wall clock minus the device stages), the share of step_s a
bank step takes - below 1 the card sustains that many live streams - and stream.py's numpy restatement of the step on the downloaded
embeddings as the yardstick.  The models carry synthetic weights: the times do not depend on them.
    python tools/stream_bench.py [--streams 1,16,64,256] [--iters 5] [--out FILE]"""
from __future__ import annotations

import argparse
import importlib
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PKG = "speaker-diarization-toolkit_amd"
STEP_S, CAPACITY, WINDOW = 0.5, 20, 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,16,64,256")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    ops, dz, rn, sg, sm = (importlib.import_module(f"{PKG}.{m}") for m in ("ops", "diarize", "resnet", "segmentation", "stream"))
    eng = ops.get_engine(0)
    diar = dz.Diarizer(eng, sg.Segmentation(eng, sg.synthetic_weights(0)), rn.ResNet34(eng, rn.synthetic_weights(0), precision=0))
    rng = np.random.default_rng(0)
    hop = int(STEP_S * 16000)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return out, a.elapsed_time(b)

    cases = []
    for R in (int(v) for v in args.streams.split(",")):
        n = sm.CHUNK + (args.iters + 2) * hop
        t = np.arange(n) / 16000.0
        pcm = [np.clip(np.round((0.1 * rng.standard_normal(n) + 0.2 * np.sin(2 * np.pi * (150 + 7 * r) * t)) * 32768), -32768, 32767).astype(np.int16)
               for r in range(R)]
        bank = diar.open_streams(R, step_s=STEP_S, capacity=CAPACITY)
        bank.push([x[:sm.CHUNK + hop] for x in pcm])                          # two warm bank steps
        whole = []
        for i in range(args.iters):                                           # whole bank steps: wall clock around one push of one hop
            a = sm.CHUNK + (i + 1) * hop
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bank.push([x[a:a + hop] for x in pcm])
            whole.append((time.perf_counter() - t0) * 1e3)
            assert len(bank.last_sync) == 1 and bank.last_sync[0]["downloads"] == 1
        # the device stages of one bank step, one by one on the bank's own buffer
        cut = torch.from_numpy((np.arange(R) * sm.SLOT).astype(np.int32)).to(eng.device)
        seg_ms, emb_ms, step_ms = [], [], []
        on = torch.ones(R, dtype=torch.uint8, device=eng.device)
        starts = torch.zeros(R, dtype=torch.int64, device=eng.device)
        state = eng.stream_state(R, CAPACITY, bank.d)
        for i in range(args.iters + 1):
            lp, a = timed(lambda: diar.seg.forward(bank.buf, cut))
            (cls, info, E), b = timed(lambda: diar.embed_chunks(bank.buf, int(bank.buf.numel()), cut, lp))
            starts.fill_(i * hop)
            _, c = timed(lambda: eng.stream_step(state, E, info, cls, starts, on, hop, hop, 1.0))
            if i:
                seg_ms.append(a), emb_ms.append(b), step_ms.append(c)
        # the step kernel alone: WINDOW launches back to back, stream r one hop further on at every launch
        ends = torch.from_numpy((np.arange(WINDOW + 10)[:, None] * hop + np.zeros((1, R), np.int64)).astype(np.int64)).to(eng.device)
        lib, s0 = eng.lib, torch.cuda.current_stream().cuda_stream

        def launch(i):
            return lib.sdk_stream_step(eng.ctx, E.data_ptr(), info.data_ptr(), cls.data_ptr(), ends.data_ptr() + 8 * R * i, on.data_ptr(), None, R,
                                       int(cls.shape[1]), bank.d, CAPACITY, hop, hop, 1.0, 2, state.buf.data_ptr(), state.nbytes, state.labels.data_ptr(),
                                       state.score.data_ptr(), state.K.data_ptr(), state.emit_lo.data_ptr(), state.emit_n.data_ptr(),
                                       state.count.data_ptr(), state.speakers.data_ptr(), s0)
        eng.stream_reset(state)
        assert all(launch(i) == 0 for i in range(10))                         # warm, and the ring in its steady state
        win_us, sub_us = [], []
        for _ in range(3):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            t0 = time.perf_counter()
            rcs = [launch(10 + i) for i in range(WINDOW)]
            t1 = time.perf_counter()
            b.record()
            torch.cuda.synchronize()
            assert not any(rcs)
            win_us.append(a.elapsed_time(b) * 1e3 / WINDOW), sub_us.append((t1 - t0) * 1e6 / WINDOW)
            eng.stream_reset(state)
            assert all(launch(i) == 0 for i in range(10))
        E_h, info_h, cls_h = E.cpu().numpy().reshape(R, 3, -1), info.cpu().numpy(), cls.cpu().numpy()
        hs = [sm.HostStream(CAPACITY, bank.d) for _ in range(R)]
        t0 = time.perf_counter()
        for r in range(R):
            sm.step_host(hs[r], E_h[r], info_h[r], cls_h[r], 0, 0)
        host_ms = (time.perf_counter() - t0) * 1e3
        w, s, e, call = (float(np.median(v)) for v in (whole, seg_ms, emb_ms, step_ms))
        k = float(np.median(win_us)) / 1e3
        cases.append({"streams": R, "bank_step_ms": w, "segmentation_ms": s, "embedding_ms": e, "step_kernel_us": 1e3 * k, "submit_us": float(np.median(sub_us)),
                      "step_call_ms": call, "host_ms": max(0.0, w - s - e - k),
                      "share_of_step": w / (STEP_S * 1e3), "numpy_step_ms": host_ms})
    line = json.dumps({"tool": "stream_bench", "step_s": STEP_S, "capacity": CAPACITY, "iters": args.iters, "window": WINDOW, "device": torch.cuda.get_device_name(0),
                       "cases": cases})
    print(line)
    if args.out:
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
