"""PyanNet segmentation forward over one hour of audio at a 1-s step (B = 3591 ten-second chunks cut on the device from a resident recording) on
one MI355X -> one JSON line.

Times sdk_segmentation_forward with HIP events after a warmup, and the stages alone the same way: the SincNet front end (sdk_sincnet_frontend),
each BiLSTM layer (sdk_bilstm_layer: input projection + recurrence) and the head (the forward minus the rest).  Roofline: FLOP from
segmentation.macs_per_chunk against the 2.5 PFLOP/s dense bf16 peak.  Yardstick, never on the product path: the same network as torch modules
on the same GPU, same process, same batch, timed the same way (MIOpen convolutions, torch's GPU nn.LSTM) in fp16, or fp32 if torch refuses
fp16 for the RNN; the format used is recorded.  MIOpen indexes tensors in int32, and the sinc conv's output of the whole batch has 4.6e9
elements, so the yardstick runs the batch as consecutive sub-batches of 512 chunks inside one timed call.
    python tools/segmentation_bench.py [--B 3591] [--warmup 1] [--iters 3] [--precision 0] [--no-yardstick] [--out FILE]"""
from __future__ import annotations

import argparse
import importlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PKG = "speaker-diarization-toolkit_amd"
PEAK_BF16 = 2.5e15


def timed(fn, warmup: int, iters: int) -> float:
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def torch_model(seg, w, dtype):
    """The same network as torch modules (the sinc filters as a fixed Conv1d weight)."""
    import numpy as np
    import torch
    import torch.nn as nn
    import torch.nn.functional as Fn

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.wav_norm = nn.InstanceNorm1d(1, affine=True)
            self.sinc = nn.Conv1d(1, 80, 251, stride=10, bias=False)
            self.convs = nn.ModuleList([nn.Conv1d(80, 60, 5), nn.Conv1d(60, 60, 5)])
            self.norms = nn.ModuleList([nn.InstanceNorm1d(80, affine=True), nn.InstanceNorm1d(60, affine=True), nn.InstanceNorm1d(60, affine=True)])
            self.lstm = nn.LSTM(60, 128, num_layers=4, bidirectional=True, batch_first=True)
            self.linear = nn.ModuleList([nn.Linear(256, 128), nn.Linear(128, 128)])
            self.classifier = nn.Linear(128, 7)

        def forward(self, x):
            x = self.sinc(self.wav_norm(x))
            x = Fn.leaky_relu(self.norms[0](Fn.max_pool1d(torch.abs(x), 3, 3)), 0.01)
            for conv, norm in zip(self.convs, self.norms[1:]):
                x = Fn.leaky_relu(norm(Fn.max_pool1d(conv(x), 3, 3)), 0.01)
            x, _ = self.lstm(x.transpose(1, 2).contiguous())
            for lin in self.linear:
                x = Fn.leaky_relu(lin(x), 0.01)
            return Fn.log_softmax(self.classifier(x), dim=-1)

    m = Net()
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in w.items() if k.startswith(("lstm.", "linear.", "classifier."))}
    sd["wav_norm.weight"], sd["wav_norm.bias"] = torch.from_numpy(w["sincnet.wav_norm1d.weight"]), torch.from_numpy(w["sincnet.wav_norm1d.bias"])
    sd["sinc.weight"] = torch.from_numpy(seg.sinc_filters(w["sincnet.conv1d.0.filterbank.low_hz_"], w["sincnet.conv1d.0.filterbank.band_hz_"])
                                         .astype(np.float32))[:, None, :]
    for i in (1, 2):
        sd[f"convs.{i - 1}.weight"], sd[f"convs.{i - 1}.bias"] = torch.from_numpy(w[f"sincnet.conv1d.{i}.weight"]), torch.from_numpy(w[f"sincnet.conv1d.{i}.bias"])
    for i in range(3):
        sd[f"norms.{i}.weight"], sd[f"norms.{i}.bias"] = torch.from_numpy(w[f"sincnet.norm1d.{i}.weight"]), torch.from_numpy(w[f"sincnet.norm1d.{i}.bias"])
    m.load_state_dict(sd)
    return m.cuda().to(dtype).eval()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=3591)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--precision", type=int, default=0)
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("segmentation_bench: no GPU visible - this tool measures the MI355X and has no CPU mode")
    ops = importlib.import_module(f"{PKG}.ops")
    seg = importlib.import_module(f"{PKG}.segmentation")
    lib = importlib.import_module(f"{PKG}._lib")
    eng = ops.get_engine(0)
    w = seg.synthetic_weights(0)
    model = seg.Segmentation(eng, w, precision=args.precision)
    B, S, F = args.B, seg.CHUNK, seg.num_frames(seg.CHUNK)
    n = S + (B - 1) * 16000
    rng = np.random.default_rng(0)
    rec = torch.from_numpy(np.clip(rng.normal(0, 3000, n), -32768, 32767).astype(np.int16)).cuda()
    starts = torch.arange(B, dtype=torch.int32, device="cuda") * 16000
    ms = timed(lambda: model.forward(rec, starts), args.warmup, args.iters)
    ms_front = timed(lambda: model.frontend(rec, starts), args.warmup, args.iters)
    x = model.frontend(rec, starts)
    ms_layers = []
    for l in range(4):
        ms_layers.append(timed(lambda: model.bilstm_layer(l, x, B, F), args.warmup, args.iters))
        x = model.bilstm_layer(l, x, B, F)
    ms_head = ms - ms_front - sum(ms_layers)
    flops = 2.0 * seg.macs_per_chunk(S) * B
    out = {"bench": "segmentation_forward", "B": B, "S": S, "F": F, "precision": args.precision, "ms": round(ms, 3),
           "chunks_per_s": round(B / (ms * 1e-3), 1), "real_time_factor": round((ms * 1e-3) / (n / 16000), 6),
           "stages_ms": {"frontend": round(ms_front, 3), **{f"lstm{l}": round(v, 3) for l, v in enumerate(ms_layers)}, "head": round(ms_head, 3)},
           "lstm_layer_us_per_step": round(float(np.mean(ms_layers)) * 1e3 / F, 3),
           "gflop_per_chunk": round(flops / B / 1e9, 4), "frac_bf16_peak": round(flops / (ms * 1e-3) / PEAK_BF16, 4),
           "frac_bf16_peak_frontend": round(2.0 * B * (seg.macs_per_chunk(S) - sum(2 * F * 512 * (d + 128) for d in (60, 256, 256, 256))
                                                      - F * (256 * 128 + 128 * 128 + 128 * 7)) / (ms_front * 1e-3) / PEAK_BF16, 4),
           "frac_bf16_peak_lstm": round(2.0 * B * sum(2 * F * 512 * (d + 128) for d in (60, 256, 256, 256)) / (sum(ms_layers) * 1e-3) / PEAK_BF16, 4),
           "device": lib.device_info(0)["name"]}
    if not args.no_yardstick:
        starts_h = np.arange(B) * 16000
        chunks = torch.stack([rec[s:s + S] for s in starts_h.tolist()]).float().reshape(B, 1, S).contiguous()
        for dt, name in ((torch.float16, "fp16"), (torch.float32, "fp32")):
            m = None
            try:
                m = torch_model(seg, w, dt)
                xin = chunks.to(dt).contiguous()
                sub = 512                                  # MIOpen indexes in int32: the sinc conv's output of 3591 chunks is 4.6e9 elements
                with torch.no_grad():
                    ms_ref = timed(lambda: [m(xin[a:a + sub]) for a in range(0, B, sub)], args.warmup, args.iters)
                out["yardstick_torch_format"] = name
                out["yardstick_sub_batch"] = sub
                out["yardstick_torch_ms"] = round(ms_ref, 3)
                out["speedup_vs_yardstick"] = round(ms_ref / ms, 3)
                break
            except RuntimeError as e:                    # torch refuses the format: record and try fp32
                out[f"yardstick_torch_{name}_error"] = str(e)[:200]
                del m
                torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
