#!/usr/bin/env python3
"""What the opt-in lossy modes cost in image space, on the SYNTHETIC weights (no checkpoint needed): PSNR / SSIM of the frames
of every mode against the f16 frames (`seva.metrics`), with the share of saturated bytes (0 or 255) beside each row -- a frame
that is mostly saturated hides differences, so the share says how much of the picture the score can see.

    python tools/kmode_quality.py [--frames 4] [--views 21] [--steps 4] [--model full|tiny]

  VAE decode   the same `frames` latents (72 x 72) through the f16 decoder and through fp8 / phases / fp8 + phases
  UNet         one one-pass window (`pipeline.run_views`: 1 input view + `views` - 1 targets, `steps` sampler steps) in f16 and in
               fp8, fp8 + fp8 attention, fp8 + fp8 feed-forward, fp8 + both; every arm decoded by the f16 VAE

Synthetic-weight numbers: they rank the modes and show that the tooling works; what a mode costs on a real checkpoint
stays unmeasured."""
import argparse
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "stable-virtual-camera_amd"))
import torch  # noqa: E402

from seva import frames, metrics, pipeline  # noqa: E402
from seva import synthetic as synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=4)
ap.add_argument("--views", type=int, default=21)
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--model", choices=("full", "tiny"), default="full")
args = ap.parse_args()
warnings.simplefilter("ignore")
dev = torch.device("cuda:0")


def vae(seed=3):
    from oracle import vae_ref as V
    from seva.modules.autoencoder import AutoEncoder
    ae = AutoEncoder(random_init=True)
    ae.module.load_state_dict(synth.synth_state_dict(V.decoder_shapes(), seed), strict=False)
    return ae.to(dev)


def unet():
    from seva.model import Seva, SevaParams
    with torch.device("meta"):
        net = Seva(SevaParams() if args.model == "full" else SevaParams(model_channels=64))
    sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 0)
    net.load_state_dict(sd, strict=True, assign=True)
    return net.to(dev).eval()


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm())


def row(name, rgb, ref_rgb):
    m = metrics.compare(rgb, ref_rgb)
    u8 = frames.to_uint8(rgb)
    sat = float(((u8 == 0) | (u8 == 255)).double().mean())
    psnr = m["psnr"]
    fin = psnr[torch.isfinite(psnr)]
    print(f"   {name:28s} rel-L2 {rel_l2(rgb, ref_rgb):.3e} | PSNR mean {float(fin.mean()) if fin.numel() else float('inf'):6.2f} dB, worst "
          f"{float(psnr.min()):6.2f} | SSIM mean {float(m['ssim'].mean()):.4f}, worst {float(m['ssim'].min()):.4f} | saturated {100 * sat:5.1f} %",
          flush=True)


with torch.no_grad():
    ae = vae()
    z = (torch.randn(args.frames, 4, 72, 72, generator=torch.Generator().manual_seed(0)) * 0.18215 * 4).to(dev)
    ref = ae.set_precision("f16").set_upsample("taps").decode(z).clone()
    print(f"== VAE decode of {args.frames} 576 x 576 frames, synthetic weights: frames of each mode against the f16 frames", flush=True)
    row("f16 taps (itself)", ref, ref)
    for p, u in (("fp8", "taps"), ("f16", "phases"), ("fp8", "phases")):
        row(f"{p} {u}", ae.set_precision(p).set_upsample(u).decode(z), ref)
    ae.set_precision("f16").set_upsample("taps")

    net = unet()
    from seva.model import SGMWrapper
    n = args.views
    c2ws, Ks = synth.orbit_c2w(n), synth.default_K(n)
    g = torch.Generator().manual_seed(23)
    lat = (torch.randn(1, 4, 72, 72, generator=g) * 0.18215 * 5.0).to(dev)
    tok = torch.randn(1024, generator=g)
    tok = (tok / tok.norm()).to(dev)

    def window(**mode):
        net.set_precision(**mode)
        res = pipeline.run_views(SGMWrapper(net), lat, c2ws, Ks, [0], clip_token=tok, T=n, num_steps=args.steps, device=dev, ae=ae)
        return res["latents"][1:].clone(), res["rgb"][1:].clone()  # (the decoder may hand out its own buffer)

    print(f"== UNet ({args.model}), one window of {n} views, {args.steps} steps, synthetic weights, f16 VAE decode: frames of each mode against "
          "the f16 frames", flush=True)
    zl, ref = window(precision="f16")
    row("f16 (itself)", ref, ref)
    for name, mode in (("fp8", dict(precision="fp8", attention="f16", ff="f16")),
                       ("fp8 + attention fp8", dict(precision="fp8", attention="fp8", ff="f16")),
                       ("fp8 + ff fp8", dict(precision="fp8", attention="f16", ff="fp8")),
                       ("fp8 + attention fp8 + ff fp8", dict(precision="fp8", attention="fp8", ff="fp8"))):
        zz, rgb = window(**mode)
        print(f"   {name:28s} latents rel-L2 {rel_l2(zz, zl):.3e}", flush=True)
        row("", rgb, ref)
