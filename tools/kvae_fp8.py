#!/usr/bin/env python3
"""The opt-in fp8 VAE decoder (AutoEncoder.set_precision("fp8"), SD-2.1 topology with the
synthetic weights of tests/test_vae_fp8_gpu.py, 576 x 576 frames) against the f16 one.

    python tools/kvae_fp8.py [--iters N] [--rounds R] [--batches 1,7,21]
    python tools/kvae_fp8.py --decode-once     # set-up, a 2 s pause, then one 7-frame fp8 decode (run it under rocprofv3 --kernel-trace)
    python tools/kvae_fp8.py --stats-from-trace KERNEL_TRACE.csv OUT.csv   # kernel stats of the launches after that pause only

1. the decoder's 3x3 conv shapes that run in e4m3 in the fp8 decode, at 7 frames per pass: us and TFLOP/s of the f16 conv and of the
   e4m3 conv (default dispatch: csrc/conv_win.hip, linear tiles at 72 px, 2-D tiles from 144 px), interleaved;
2. whole-decode ms/frame at 1 / 7 / 21 frames per pass, f16, fp8 and fp8 with the e4m3 upsample convs (SEVA_VAE_FP8_UPSAMPLE=1)
   interleaved on the same AutoEncoder, and the rel-L2 of each fp8 decode to the f16 one."""
import argparse
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stable-virtual-camera_amd"), ROOT]
import torch  # noqa: E402

from oracle import vae_ref  # noqa: E402
from seva import ops, synthetic  # noqa: E402
from seva.modules.autoencoder import AutoEncoder  # noqa: E402

warnings.simplefilter("ignore")
dev = torch.device("cuda:0")
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batches", default="1,7,21")
ap.add_argument("--decode-once", action="store_true")
ap.add_argument("--stats-from-trace", nargs=2, metavar=("KERNEL_TRACE_CSV", "OUT_CSV"))
args = ap.parse_args()

if args.stats_from_trace:
    # rocprofv3's kernel stats cover the whole process (engine set-up and weight packing included): keep the launches after the
    # longest gap between launches (the --decode-once pause) and aggregate them in rocprofv3's kernel_stats.csv columns
    import csv

    src, dst = args.stats_from_trace
    rows = sorted(csv.DictReader(open(src)), key=lambda r: int(r["Start_Timestamp"]))
    gaps = [int(b["Start_Timestamp"]) - int(a["End_Timestamp"]) for a, b in zip(rows, rows[1:])]
    cut = max(range(len(gaps)), key=gaps.__getitem__)
    if gaps[cut] < 1e9:
        sys.exit(f"no pause of >= 1 s in {src}: not a --decode-once trace")
    per = {}
    for r in rows[cut + 1:]:
        per.setdefault(r["Kernel_Name"], []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    total = sum(sum(v) for v in per.values())
    with open(dst, "w", newline="") as f:
        w = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
        w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage", "MinNs", "MaxNs"])
        for name, d in sorted(per.items(), key=lambda kv: -sum(kv[1])):
            w.writerow([name, len(d), sum(d), sum(d) / len(d), round(100.0 * sum(d) / total, 2), min(d), max(d)])
    print(f"{len(rows) - cut - 1} launches after a {gaps[cut] / 1e9:.2f} s pause ({cut + 1} set-up launches dropped), "
          f"{total / 1e6:.2f} ms of kernel time -> {dst}")
    sys.exit(0)

ae = AutoEncoder(random_init=True)
ae.module.load_state_dict(synthetic.synth_state_dict(vae_ref.decoder_shapes(), 3), strict=False)  # the GPU tests' synthetic weights
ae = ae.to(dev)
g = torch.Generator().manual_seed(0)
batches = [int(v) for v in args.batches.split(",")]
zall = (torch.randn(max(batches + [7]), 4, 72, 72, generator=g) * 0.18215 * 4).to(dev)

if args.decode_once:
    ae.set_precision("fp8")
    ae.engine().fp8_weights()  # pack the e4m3 weights first: the decode below is the only one
    torch.cuda.synchronize()
    time.sleep(2.0)  # marks the end of the set-up in a kernel trace (--stats-from-trace)
    with torch.no_grad():
        out = ae.decode(zall[:7])
    torch.cuda.synchronize()
    print(f"one fp8 decode of 7 frames: {tuple(out.shape)}, finite: {bool(torch.isfinite(out).all())}", flush=True)
    sys.exit(0)


def timeit(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


print("== decoder convs that run in e4m3, 7 frames per pass: side cin cout up x calls | us f16 (TFLOP/s) | us e4m3 (TFLOP/s) | e4m3 / f16",
      flush=True)
tot16 = tot8 = 0.0
n = 7
for side, cin, cout, up, calls in [(72, 512, 512, False, 10), (144, 512, 512, False, 6), (288, 512, 256, False, 1), (288, 256, 256, False, 4),
                                   (576, 256, 128, False, 1), (576, 128, 128, False, 4), (72, 512, 512, True, 1), (144, 512, 512, True, 1),
                                   (288, 256, 256, True, 1)]:
    s = 2 if up else 1
    M = n * (s * side) ** 2
    x = torch.randn(n, side, side, cin, device=dev)
    w = torch.randn(cout, 9 * cin, device=dev) * 0.02
    x16, w16 = x.half(), w.half()
    x8 = ops.to_fp8(x)
    w8, e8 = ops.quantize_weight_fp8(w)
    del x, w
    b = torch.randn(cout, device=dev)
    out = torch.empty(n, (s * side) ** 2, cout, device=dev)
    st = torch.empty(ops.channel_stats_shape(M, cout), device=dev)
    best16 = best8 = 1e30
    for _ in range(args.rounds):
        best16 = min(best16, timeit(lambda: ops.conv3x3(x16, w16, bias=b, out_f32=out, ch_stats=st, upsample=up), args.iters))
        best8 = min(best8, timeit(lambda: ops.conv3x3(x8, w8, w_exp=e8, bias=b, out_f32=out, ch_stats=st, upsample=up), args.iters))
    fl = 2.0 * M * cout * 9 * cin
    tot16 += best16 * calls / 1e3
    tot8 += best8 * calls / 1e3
    print(f"{side:4d} {cin:4d} {cout:4d} {'up' if up else '  '} x{calls:2d} | {best16:9.1f} ({fl / best16 / 1e6:6.1f}) | {best8:9.1f} ({fl / best8 / 1e6:6.1f}) "
          f"| {best8 / best16:5.2f}", flush=True)
    del x16, w16, x8, w8, out, st
torch.cuda.empty_cache()
print(f"   these convs per 7-frame pass: f16 {tot16:.2f} ms, e4m3 {tot8:.2f} ms ({tot16 / n:.2f} -> {tot8 / n:.2f} ms/frame)", flush=True)

print("== whole decode, f16 / fp8 / fp8 + e4m3 upsample convs interleaved (best of rounds)", flush=True)
eng = ae.engine()
eng.fp8_upsample = False
w8_default = eng.fp8_weights()
eng.fp8_upsample, eng.W8 = True, None
w8_up = eng.fp8_weights()
variants = {"f16": ("f16", None), "fp8": ("fp8", w8_default), "fp8+up": ("fp8", w8_up)}
for nb in batches:
    z = zall[:nb]
    best = {k: 1e30 for k in variants}
    outs = {}
    for r in range(args.rounds):
        for name, (prec, w8) in variants.items():
            ae.set_precision(prec)
            if w8 is not None:
                eng.W8 = w8
            with torch.no_grad():
                if r == 0:
                    outs[name] = eng.decode(z, ae.scale_factor)
                torch.cuda.synchronize()
                reps = 3 if nb < 8 else 1
                t0 = time.perf_counter()
                for _ in range(reps):
                    eng.decode(z, ae.scale_factor)
                torch.cuda.synchronize()
            best[name] = min(best[name], (time.perf_counter() - t0) / reps)
    ref = outs["f16"].double()
    err = {k: float((outs[k].double() - ref).norm() / ref.norm()) for k in ("fp8", "fp8+up")}
    print(f"decode {nb:2d} frames per pass: f16 {best['f16'] * 1e3 / nb:6.2f} ms/frame | fp8 {best['fp8'] * 1e3 / nb:6.2f} ms/frame "
          f"({best['fp8'] / best['f16']:.3f}x, rel-L2 {err['fp8']:.3e}) | fp8 + e4m3 upsample {best['fp8+up'] * 1e3 / nb:6.2f} ms/frame "
          f"({best['fp8+up'] / best['f16']:.3f}x, rel-L2 {err['fp8+up']:.3e}) | arena {eng.arena.nbytes() / 2**30:.2f} GiB", flush=True)
    del outs
    torch.cuda.empty_cache()
