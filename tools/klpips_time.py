"""Device time of LPIPS (`metrics.LPIPS`: VGG-16 tower + layer distances of 168 pairs of 576 x 576 frames, synthetic weights) and of
its own three operators alone (no threshold: scoring is not on the sampler's critical path; DESIGN.md quotes it).
Run from the repository root on an MI355X:  python tools/klpips_time.py"""
import sys

import torch

sys.path.insert(0, "stable-virtual-camera_amd")
from seva import metrics, ops  # noqa: E402
from seva import synthetic as synth  # noqa: E402
from seva._lpips_engine import pair_bytes  # noqa: E402

dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
n, H, W = 168, 576, 576


def device_ms(fn):
    fn()  # warm-up: code object load, allocator, the engine's arena
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


w = metrics.LpipsWeights()
w.load_state_dict(synth.synth_lpips_state_dict({k: tuple(v.shape) for k, v in w.state_dict().items()}, 0))
m = metrics.LPIPS(w).to(dev)
ua = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.int64).to(torch.uint8).to(dev)
ub = (ua.to(torch.int16) + torch.randint(-12, 13, ua.shape, generator=g).to(torch.int16).to(dev)).clamp(0, 255).to(torch.uint8)

res = {}
t_all = device_ms(lambda: res.__setitem__("lpips", m(ua, ub)))
cs = m.engine()._chunk(n, H, W)
lp = res["lpips"]
print(f"LPIPS (VGG-16) of {n} pairs of {W}x{H} uint8 frames: {t_all:.1f} ms ({t_all / n:.2f} ms per pair), {cs} pairs per pass, "
      f"arena {m.engine().arena.nbytes() / 2**30:.2f} GiB ({pair_bytes(H, W) / 2**20:.0f} MiB per pair); scores "
      f"{float(lp.min()):.3e} .. {float(lp.max()):.3e}, finite {bool(torch.isfinite(lp).all())}", flush=True)
t_psnr = device_ms(lambda: metrics.compare(ua, ub))
print(f"  beside it: squared error + SSIM of the same frames {t_psnr:.2f} ms", flush=True)

# the three operators alone, on one pass's worth of frames (2 * cs frames)
k = 2 * cs
x0 = torch.empty((k, H, W, 64), dtype=torch.float16, device=dev)
t_prep = device_ms(lambda: ops.lpips_prepare(ua[:k], x0))
x0.normal_()
p0 = torch.empty((k, H // 2, W // 2, 64), dtype=torch.float16, device=dev)
t_relu = device_ms(lambda: ops.lpips_relu_pool(x0, x0))
t_pool = device_ms(lambda: ops.lpips_relu_pool(x0, x0, p0))
gb = k * H * W * 64 * 2 / 1e9
print(f"  prepare {k} frames {t_prep:.3f} ms ({gb / t_prep * 1e3:.0f} GB/s written); ReLU in place {t_relu:.3f} ms "
      f"({2 * gb / t_relu * 1e3:.0f} GB/s); ReLU + pool {t_pool:.3f} ms ({2.25 * gb / t_pool * 1e3:.0f} GB/s)", flush=True)
out = torch.empty(cs, dtype=torch.float64, device=dev)
for C, side in ((64, 576), (128, 288), (256, 144), (512, 72), (512, 36)):
    f = torch.randn((k, side * side, C), device=dev).relu().half()
    wl = torch.rand(C, device=dev) / C
    ws = torch.empty(ops.lpips_layer_workspace_numel(cs, side * side), dtype=torch.uint8, device=dev)
    t = device_ms(lambda: ops.lpips_layer(f[:cs], f[cs:], wl, out, ws))
    print(f"  layer distance C={C} {side}x{side}, {cs} pairs: {t:.3f} ms ({f.numel() * 2 / 1e9 / t * 1e3:.0f} GB/s read)", flush=True)
    del f
