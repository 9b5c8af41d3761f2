#!/usr/bin/env python3
"""The VAE decoder's three upsample convs (72 -> 144 and 144 -> 288 at 512 channels, 288 -> 576 at 256) as four 2x2 phase convs
(`ops.conv3x3_up_phases128`, seva_gemm_desc.upsample = 4) against the nine-tap fused-upsample conv (`ops.conv3x3(upsample=True)`),
and the decode with `AutoEncoder.set_upsample("phases")` against the default.

    python tools/kvae_up_phases.py conv     [--frames 7] [--iters 10] [--rounds 3]
    python tools/kvae_up_phases.py decode   [--frames 7] [--iters 3]  [--rounds 3] [--taps-only]
    python tools/kvae_up_phases.py accuracy

conv:     exactness on integer data, then interleaved timing per conv, both arms WITH GroupNorm statistics (as the decoder calls
          them): best of R rounds and max - min over the rounds per arm, default dispatch / 4-wave / 8-wave family, ratio phases / nine-tap.
decode:   ms per 576 x 576 frame at `frames` per pass, f16 and fp8 decode x taps and phases, arms interleaved in every round.
          --taps-only: the default path alone (run it with SEVA_HIP_LIB=<the parent's library> to see that it did not move).
accuracy: rel-L2 of a 576 x 576 and a 768 x 576 frame: phases against taps, and both against oracle/vae_ref.py (CPU, slow)."""
import argparse
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "stable-virtual-camera_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from seva import ops  # noqa: E402
from seva._engine import combine_up_phases, pack_conv3x3  # noqa: E402

dev = torch.device("cuda:0")
ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("conv", "decode", "accuracy"))
ap.add_argument("--frames", type=int, default=7)
ap.add_argument("--iters", type=int, default=0)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--taps-only", action="store_true")
args = ap.parse_args()
warnings.simplefilter("ignore")


def timeit(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm())


def vae(seed=3):
    from oracle import vae_ref as V
    from seva import synthetic as synth
    from seva.modules.autoencoder import AutoEncoder
    ae = AutoEncoder(random_init=True)
    sd = synth.synth_state_dict(V.decoder_shapes(), seed)
    ae.module.load_state_dict(sd, strict=False)
    return ae.to(dev), sd


def mode_conv():
    iters = args.iters or 10
    nbad = 0
    for k, (n, ih, iw, cin, cout) in enumerate([(3, 8, 8, 64, 128), (2, 8, 72, 64, 128), (2, 16, 144, 64, 128), (1, 8, 96, 128, 256)]):
        g = torch.Generator().manual_seed(k)
        x = torch.randint(-3, 4, (n, cin, ih, iw), generator=g).float().to(dev)
        w = torch.randint(-2, 3, (cout, cin, 3, 3), generator=g).float().to(dev)
        ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1).permute(0, 2, 3, 1).reshape(n, 4 * ih * iw, cout)
        xh, w4 = x.permute(0, 2, 3, 1).contiguous().half(), combine_up_phases(w)
        bad = []
        for knob in (-1, 1, 2):
            ops.set_knob("conv_win", knob)
            out = torch.full((n, 4 * ih * iw, cout), float("nan"), device=dev)
            ops.conv3x3_up_phases128(xh, w4, out_f32=out)
            torch.cuda.synchronize()
            if not torch.equal(out, ref):
                bad.append(knob)
        nbad += len(bad)
        print(f"exact {(n, ih, iw, cin, cout)}: {'OK' if not bad else 'MISMATCH, knobs ' + str(bad)}", flush=True)
    ops.set_knob("conv_win", -1)
    n = args.frames
    print(f"== VAE upsample convs at {n} frames, both arms with ch_stats, {args.rounds} interleaved rounds of {iters} calls: best us (max - min "
          "over the rounds)", flush=True)
    print("   source -> output, channels | nine-tap (TFLOP/s) | phases, default dispatch (TFLOP/s) | phases 4-wave | phases 8-wave | phases / nine-tap", flush=True)
    tot = {"9": 0.0, -1: 0.0}
    for side, c in [(72, 512), (144, 512), (288, 256)]:
        M = n * 4 * side * side
        x = torch.randn(n, side, side, c, device=dev, dtype=torch.float16)
        w = torch.randn(c, c, 3, 3, device=dev) * 0.02
        w9, w4 = pack_conv3x3(w), combine_up_phases(w)
        b = torch.randn(c, device=dev)
        out = torch.empty(n, 4 * side * side, c, device=dev)
        st = torch.empty(ops.channel_stats_shape(M, c), device=dev)
        t = {"9": [], -1: [], 1: [], 2: []}

        def nine():
            ops.set_knob("conv_win", -1)
            ops.conv3x3(x, w9, upsample=True, bias=b, out_f32=out, ch_stats=st)

        def phases(knob):
            ops.set_knob("conv_win", knob)
            ops.conv3x3_up_phases128(x, w4, bias=b, out_f32=out, ch_stats=st, alg_k=9 * c)

        for _ in range(args.rounds):
            t["9"].append(timeit(nine, iters))
            for knob in (-1, 1, 2):
                t[knob].append(timeit(lambda: phases(knob), iters))
        fl = 2.0 * M * c * 9 * c
        f = {k: f"{min(v):8.1f} ({max(v) - min(v):5.1f})" for k, v in t.items()}
        tot["9"] += min(t["9"])
        tot[-1] += min(t[-1])
        print(f"{side:3d} -> {2 * side:3d} {c:4d} | {f['9']} ({fl / min(t['9']) / 1e6:6.1f}) | {f[-1]} ({fl / min(t[-1]) / 1e6:6.1f}) | {f[1]} | {f[2]} | "
              f"{min(t[-1]) / min(t['9']):.3f}", flush=True)
        del x, out, st
    print(f"   the three convs: nine-tap {tot['9'] / 1e3:.3f} ms, phases {tot[-1] / 1e3:.3f} ms ({(tot['9'] - tot[-1]) / 1e3 / n:.3f} ms per frame less), "
          f"ratio {tot[-1] / tot['9']:.3f}", flush=True)
    ops.set_knob("conv_win", -1)
    return nbad


def mode_decode():
    iters = args.iters or 3
    n = args.frames
    ae, _ = vae()
    z = (torch.randn(n, 4, 72, 72, generator=torch.Generator().manual_seed(0)) * 0.18215 * 4).to(dev)
    arms = [(p, u) for p in ("f16", "fp8") for u in (("taps",) if args.taps_only else ("taps", "phases"))]
    t = {a: [] for a in arms}
    eng = ae.engine()

    # which GroupNorms behind an upsample conv run their own statistics pass (no statistics from the producer)
    own = {a: [] for a in arms}
    real_gn = ops.groupnorm
    watch, cur = set(), [None]

    def gn(x1, *a, **k):
        if x1.data_ptr() in watch:
            own[cur[0]].append(k.get("stats1") is None)
        return real_gn(x1, *a, **k)

    ops.groupnorm = gn
    for a in arms:
        ae.set_precision(a[0]).set_upsample(a[1])
        cur[0] = a
        eng.decode(z, ae.scale_factor)
        watch.update(t_.data_ptr() for k_, t_ in eng.arena.bufs.items() if k_[0].startswith("out:") and k_[0].endswith("upsamplers.0.conv"))
        own[a] = []
        eng.decode(z, ae.scale_factor)
    ops.groupnorm = real_gn
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for a in arms:
            ae.set_precision(a[0]).set_upsample(a[1])
            t[a].append(timeit(lambda: eng.decode(z, ae.scale_factor), iters) / 1e3 / n)
    lib = os.environ.get("SEVA_HIP_LIB", "(in-tree library)")
    print(f"== VAE decode of {n} 576 x 576 frames per pass, {args.rounds} interleaved rounds of {iters} decodes, library {lib}: ms per frame, best "
          "(max - min over the rounds)", flush=True)
    for a in arms:
        print(f"   {a[0]:3s} {a[1]:6s}: {min(t[a]):6.3f} ({max(t[a]) - min(t[a]):5.3f})   GroupNorms behind the upsample convs that ran their own "
              f"statistics pass: {sum(own[a])} of {len(own[a])}", flush=True)
    if not args.taps_only:
        for p in ("f16", "fp8"):
            print(f"   {p}: phases - taps = {min(t[(p, 'phases')]) - min(t[(p, 'taps')]):+.3f} ms per frame", flush=True)
    return 0


def mode_accuracy():
    from oracle import vae_ref as V
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ae, sd = vae()
    for h, w in ((72, 72), (96, 72)):
        z = torch.randn(1, 4, h, w, generator=torch.Generator().manual_seed(12)) * 0.18215 * 4
        t0 = time.perf_counter()
        ref = V.vae_decode(sd, z)
        print(f"== {8 * h} x {8 * w} frame (oracle: {time.perf_counter() - t0:.0f} s on the CPU)", flush=True)
        for p in ("f16", "fp8"):
            ae.set_precision(p)
            taps = ae.set_upsample("taps").decode(z.to(dev)).cpu()
            ph = ae.set_upsample("phases").decode(z.to(dev)).cpu()
            print(f"   {p}: phases vs taps {rel_l2(ph, taps):.3e} | taps vs oracle {rel_l2(taps, ref):.3e} | phases vs oracle {rel_l2(ph, ref):.3e}", flush=True)
    return 0


with torch.no_grad():
    sys.exit(1 if {"conv": mode_conv, "decode": mode_decode, "accuracy": mode_accuracy}[args.mode]() else 0)
