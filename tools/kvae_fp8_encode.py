#!/usr/bin/env python3
"""The opt-in fp8 VAE encoder (AutoEncoder.set_precision(..., encode="fp8"), SD-2.1 topology with the synthetic weights of
tests/test_vae_fp8_encode_gpu.py, 576 x 576 frames) against the f16 one.

    python tools/kvae_fp8_encode.py [--iters N] [--rounds R] [--batches 1,7]
    python tools/kvae_fp8_encode.py --encode-once   # set-up, a 2 s pause, then one 7-frame fp8 encode with the e4m3 downsample convs
                                                    # (run it under rocprofv3 --kernel-trace; tools/kvae_fp8.py --stats-from-trace)

1. the encoder's three Downsample2D convs (3x3, stride 2, bottom / right padding) at 7 frames per pass: us of the e4m3 stride-2 window
   kernel (conv_win knob 1), of the e4m3 per-tap gather (the default dispatch) and of the f16 per-tap gather, interleaved;
2. whole-encode ms/frame at 1 / 7 frames per pass, f16, fp8 and fp8 with the e4m3 downsample convs (SEVA_VAE_FP8_DOWNSAMPLE=1),
   interleaved, and the rel-L2 of each fp8 encode's latents to the f16 ones."""
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
ap.add_argument("--batches", default="1,7")
ap.add_argument("--encode-once", action="store_true")
args = ap.parse_args()


def make_ae(precision, downsample):
    os.environ["SEVA_VAE_FP8_DOWNSAMPLE"] = "1" if downsample else "0"  # read when the encoder engine is built (below)
    ae = AutoEncoder(random_init=True)
    ae.module.load_state_dict(synthetic.synth_state_dict({**vae_ref.decoder_shapes(), **vae_ref.encoder_shapes()}, 3))
    ae = ae.to(dev).set_precision("f16", encode=precision)
    ae.encoder_engine()
    return ae


g = torch.Generator().manual_seed(0)
batches = [int(v) for v in args.batches.split(",")]
x = (torch.rand(max(batches + [7]), 3, 576, 576, generator=g) * 2 - 1).to(dev)

if args.encode_once:
    ae = make_ae("fp8", True)
    ae.encoder_engine().fp8_weights()
    torch.cuda.synchronize()
    time.sleep(2.0)  # marks the end of the set-up in a kernel trace
    with torch.no_grad():
        z = ae.encoder_engine().encode(x[:7], ae.scale_factor)
    torch.cuda.synchronize()
    print(f"one fp8 encode (e4m3 downsample) of 7 frames: {tuple(z.shape)}, finite: {bool(torch.isfinite(z).all())}", flush=True)
    sys.exit(0)


def timeit(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


# ---- 1. per-conv A/B of the three downsample convs, 7 frames per pass
n = 7
print(f"downsample convs, {n} frames per pass (us; e4m3 window = conv_win knob 1, e4m3 gather = the default dispatch)")
for ih, c in ((576, 128), (288, 256), (144, 512)):
    oh = ih // 2
    x8 = ops.to_fp8(torch.randn(n, ih, ih, c, device=dev))
    x16 = torch.randn(n, ih, ih, c, device=dev).half()
    w8, e8 = ops.quantize_weight_fp8(torch.randn(c, 9 * c, device=dev) * 0.02)
    w16 = (torch.randn(c, 9 * c, device=dev) * 0.02).half()
    bias = torch.randn(c, device=dev)
    out = torch.empty((n, oh * oh, c), device=dev)
    st = torch.empty(ops.channel_stats_shape(n * oh * oh, c), device=dev)

    def win():
        ops.set_knob("conv_win", 1)
        try:
            ops.conv3x3(x8, w8, w_exp=e8, stride=2, pad_br_only=True, bias=bias, out_f32=out, ch_stats=st)
        finally:
            ops.set_knob("conv_win", -1)

    def gat8():
        ops.conv3x3(x8, w8, w_exp=e8, stride=2, pad_br_only=True, bias=bias, out_f32=out, ch_stats=st)

    def gat16():
        ops.conv3x3(x16, w16, stride=2, pad_br_only=True, bias=bias, out_f32=out, ch_stats=st)

    res = {"e4m3 window": [], "e4m3 gather": [], "f16 gather": []}
    for _ in range(args.rounds):
        for k, fn in (("e4m3 window", win), ("e4m3 gather", gat8), ("f16 gather", gat16)):
            res[k].append(timeit(fn, 20) * 1e6)
    flops = 2.0 * n * oh * oh * c * 9 * c
    print(f"  {ih}^2 -> {oh}^2 x {c}: " + ", ".join(f"{k} {min(v):7.1f} us ({flops / min(v) / 1e6:6.1f} TFLOP/s)" for k, v in res.items()))

# ---- 2. whole encode
aes = {"f16": make_ae("f16", False), "fp8": make_ae("fp8", False), "fp8+downsample": make_ae("fp8", True)}
for b in batches:
    xb = x[:b]
    with torch.no_grad():
        ref = aes["f16"].encoder_engine().encode(xb, 0.18215)
        errs = {k: float(((a.encoder_engine().encode(xb, 0.18215) - ref).double().norm() / ref.double().norm())) for k, a in aes.items()}
    times = {k: [] for k in aes}
    for _ in range(args.rounds):
        for k, a in aes.items():
            eng = a.encoder_engine()
            with torch.no_grad():
                times[k].append(timeit(lambda: eng.encode(xb, 0.18215), args.iters) * 1e3 / b)
    print(f"encode 576^2, {b} frame(s) per pass: " + ", ".join(f"{k} {min(v):.3f} ms/frame" for k, v in times.items())
          + " | rel-L2 to f16: " + ", ".join(f"{k} {errs[k]:.3e}" for k in aes if k != "f16"), flush=True)
