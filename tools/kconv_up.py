#!/usr/bin/env python3
"""The three Upsample convs of a 576 x 576 step (36 -> 72 at 640 channels, 18 -> 36 and 9 -> 18 at 1280) at the CFG batch of 42:
the nine-tap fused-upsample window kernel (`ops.conv3x3(upsample=True)`, with its GroupNorm statistics where the step emits them)
against the four 2x2 phase convs (`ops.conv3x3_up_phases`, seva_gemm_desc.upsample = 2), which do 4/9 of the FLOPs.

    python tools/kconv_up.py [--iters N] [--rounds R] [--batch B]

1. exactness of the phase path on integer data against torch, default dispatch and both families;
2. interleaved timing, best of R rounds: nine-tap | phases by default dispatch | 4-wave family | 8-wave family, and the ratio
   phases / nine-tap (expected from the FLOP count: 0.45 - 0.55).  TFLOP/s are reference-equivalent (nine taps) for both."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stable-virtual-camera_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from seva import ops  # noqa: E402
from seva._engine import combine_up_phases, pack_conv3x3  # noqa: E402

dev = torch.device("cuda:0")
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batch", type=int, default=42)
ap.add_argument("--skip-exact", action="store_true")
args = ap.parse_args()


def ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float().to(dev)


nbad = 0
if not args.skip_exact:
    for k, (n, ih, iw, cin, cout) in enumerate([(2, 36, 36, 64, 640), (3, 18, 18, 128, 320), (42, 9, 9, 64, 160), (5, 7, 5, 128, 160), (1, 72, 72, 64, 160)]):
        x, w, b = ints((n, cin, ih, iw), -3, 3, 10 * k), ints((cout, cin, 3, 3), -2, 2, 10 * k + 1), ints((cout,), -4, 4, 10 * k + 2)
        ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1).permute(0, 2, 3, 1).reshape(n, 4 * ih * iw, cout)
        xh, w4 = x.permute(0, 2, 3, 1).contiguous().half(), combine_up_phases(w)
        bad = []
        for knob in (-1, 1, 2):
            ops.set_knob("conv_win", knob)
            out = torch.full((n, 4 * ih * iw, cout), float("nan"), device=dev)
            ops.conv3x3_up_phases(xh, w4, bias=b, out_f32=out)
            torch.cuda.synchronize()
            if not torch.equal(out, ref):
                bad.append((knob, float((out - ref).abs().nan_to_num(1e9).max())))
        nbad += len(bad)
        print(f"exact {(n, ih, iw, cin, cout)}: {'OK' if not bad else 'MISMATCH ' + str(bad)}", flush=True)
    ops.set_knob("conv_win", -1)


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


n = args.batch
print(f"== Upsample convs at batch {n}: source side, channels | us nine-tap (TFLOP/s) | us phases, default dispatch (TFLOP/s) | 4-wave | 8-wave | phases / nine-tap", flush=True)
tot9 = tot4 = 0.0
for side, c in [(36, 640), (18, 1280), (9, 1280)]:
    M = n * 4 * side * side
    x = torch.randn(n, side, side, c, device=dev, dtype=torch.float16)
    w = torch.randn(c, c, 3, 3, device=dev) * 0.02
    w9, w4 = pack_conv3x3(w), combine_up_phases(w)
    b = torch.randn(c, device=dev)
    out = torch.empty(n, 4 * side * side, c, device=dev)
    # the step's nine-tap call emits GroupNorm statistics where the output has whole 64-pixel blocks per image (36 -> 72 only)
    st = torch.empty(ops.channel_stats_shape(M, c), device=dev) if (4 * side * side) % ops.STATS_ROWS == 0 else None
    best = {"9": 1e30, -1: 1e30, 1: 1e30, 2: 1e30}

    def nine():
        ops.set_knob("conv_win", -1)
        ops.conv3x3(x, w9, upsample=True, bias=b, out_f32=out, ch_stats=st)

    def phases(knob):
        ops.set_knob("conv_win", knob)
        ops.conv3x3_up_phases(x, w4, bias=b, out_f32=out, alg_k=9 * c)

    for _ in range(args.rounds):
        best["9"] = min(best["9"], timeit(nine, args.iters))
        for knob in (-1, 1, 2):
            best[knob] = min(best[knob], timeit(lambda: phases(knob), args.iters))
    fl = 2.0 * M * c * 9 * c
    tot9 += best["9"]
    tot4 += best[-1]
    print(f"{side:3d} -> {2 * side:3d} {c:5d} | {best['9']:8.1f} ({fl / best['9'] / 1e6:6.1f}) | {best[-1]:8.1f} ({fl / best[-1] / 1e6:6.1f}) | {best[1]:8.1f} | {best[2]:8.1f} | "
          f"{best[-1] / best['9']:.3f}", flush=True)
    del x, out, st
print(f"   the three Upsample convs of a step: nine-tap {tot9 / 1e3:.3f} ms, phases {tot4 / 1e3:.3f} ms, ratio {tot4 / tot9:.3f}", flush=True)
ops.set_knob("conv_win", -1)
sys.exit(1 if nbad else 0)
