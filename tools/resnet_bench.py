"""ResNet34 forward at config #2's shape (B = 1000 two-second segments, T = 201 frames) on one MI355X -> one JSON line.

Times sdk_resnet_forward (features already on the device) with HIP events after a warmup; the per-kernel-family split comes from the library's
own event profile (sdk_profile_begin / _end) in a separate pass.  Yardstick, never on the product path: the same network as torch.nn in bf16,
channels_last, on the GPU (MIOpen convolutions), timed the same way.  Roofline figures: FLOP from ResNetConfig.macs_per_segment against the
2.5 PFLOP/s dense bf16 peak; compulsory layer-boundary HBM bytes (every conv reads its input - and its residual / shortcut input - and writes its
output once, 2-byte elements) against 6.3 TB/s.
    python tools/resnet_bench.py [--B 1000] [--T 201] [--warmup 3] [--iters 10] [--no-yardstick] [--out FILE]"""
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
HBM_BPS = 6.3e12


def boundary_bytes(cfg, T: int) -> int:
    """Compulsory HBM bytes of one segment's layer boundaries (features read once by the stem, then every conv's input, residual / shortcut input
    and output once, 2-byte elements); pooling reads the last map once."""
    sz = cfg.map_sizes(T)
    F, Tl = sz[0]
    tot = F * Tl * 2 + F * Tl * cfg.widths[0] * 2
    cin = cfg.widths[0]
    for l, (nb, w) in enumerate(zip(cfg.blocks, cfg.widths)):
        Fi, Ti = sz[l]
        Fo, To = sz[l + 1]
        for j in range(nb):
            xin = (Fi * Ti * cin if j == 0 else Fo * To * w) * 2
            o = Fo * To * w * 2
            tot += (xin + o) + (o + o + xin)
        cin = w
    Fo, To = sz[-1]
    return tot + Fo * To * cfg.widths[-1] * 2


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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1000)
    ap.add_argument("--T", type=int, default=201)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--precision", type=int, default=0)
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("resnet_bench: no GPU visible - this tool measures the MI355X and has no CPU mode")
    ops = importlib.import_module(f"{PKG}.ops")
    RN = importlib.import_module(f"{PKG}.resnet")
    lib = importlib.import_module(f"{PKG}._lib")
    eng = ops.get_engine(0)
    cfg = RN.DEFAULT_RESNET
    w = RN.synthetic_weights(0)
    rn = RN.ResNet34(eng, w, precision=args.precision)
    B, T = args.B, args.T
    dt = torch.float16 if args.precision == 2 else torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    feats = torch.zeros(B * T, 128, dtype=dt, device="cuda")
    feats[:, :cfg.n_feats] = (torch.randn(B * T, cfg.n_feats, device="cuda", generator=g) * 3).to(dt)
    ms = timed(lambda: rn.forward(feats, B, T), args.warmup, args.iters)
    eng.profile_begin()
    rn.forward(feats, B, T)
    torch.cuda.synchronize()
    prof = eng.profile_end()
    flops = 2.0 * cfg.macs_per_segment(T) * B
    hbm = boundary_bytes(cfg, T) * B
    out = {"bench": "resnet34_forward", "B": B, "T": T, "precision": args.precision, "ms": round(ms, 3),
           "segment_embeddings_per_s": round(B / (ms * 1e-3), 1), "gflop_per_segment": round(flops / B / 1e9, 4),
           "frac_bf16_peak": round(flops / (ms * 1e-3) / PEAK_BF16, 4),
           "hbm_boundary_mb_per_segment": round(hbm / B / 1e6, 2), "hbm_roofline_ms": round(hbm / HBM_BPS * 1e3, 3),
           "frac_hbm_roofline": round(hbm / HBM_BPS * 1e3 / ms, 4),
           "kernels_ms": {k: round(v["ms"], 3) for k, v in prof.items()}, "kernels_launches": {k: v["launches"] for k, v in prof.items()},
           "device": lib.device_info(0)["name"]}
    if not args.no_yardstick:
        sys.path.insert(0, str(ROOT / "tests"))
        ref = importlib.import_module("resnet_ref")
        m = ref.torch_resnet34(w, dtype=torch.float32).cuda().to(torch.bfloat16).to(memory_format=torch.channels_last)
        x = feats[:, :cfg.n_feats].to(torch.bfloat16).reshape(B, T, cfg.n_feats)
        with torch.no_grad():
            ms_ref = timed(lambda: m(x), args.warmup, args.iters)
        out["yardstick_torch_bf16_channels_last_ms"] = round(ms_ref, 3)
        out["speedup_vs_yardstick"] = round(ms_ref / ms, 3)
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
