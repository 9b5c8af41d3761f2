"""Device time of the two frame kernels beside the same torch expressions on the host (no threshold; DESIGN.md quotes it):
a 4032 x 3024 RGBA picture -> 576 x 576 frame (`frames.load_img_and_K`) and 168 decoded 576 x 576 frames -> uint8
(`frames.to_uint8`).  Run from the repository root on an MI355X:  python tools/kframes_time.py"""
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, "stable-virtual-camera_amd")
from seva import frames, ops  # noqa: E402

dev = torch.device("cuda:0")
torch.set_num_threads(min(16, torch.get_num_threads()))
g = torch.Generator().manual_seed(0)


def device_ms(fn):
    fn()  # warm-up: code object load, allocator
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def host_ms(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


# ---- load: 4032 x 3024 RGBA -> 576 x 576
h, w, size = 3024, 4032, (576, 576)
pic = torch.randint(0, 256, (h, w, 4), generator=g, dtype=torch.uint8)
p = frames.plan_load(h, w, size)
src, out = pic.to(dev)[None], torch.empty(1, 3, p.H, p.W, device=dev)
kw = dict(rh=p.rh, rw=p.rw, ct=p.ct - p.pt, cl=p.cl - p.pl, pad_value=1.0, out_mul=2.0, out_add=-1.0)
t_dev = device_ms(lambda: ops.image_area_crop(src, out, **kw))


def host_load():
    v = pic.float() / 255
    v = (v[..., :3] * v[..., 3:] + (1 - v[..., 3:])).permute(2, 0, 1)[None]
    v = F.interpolate(v, (p.rh, p.rw), mode="area")
    return v[:, :, p.ct:p.ct + p.H, p.cl:p.cl + p.W] * 2.0 - 1.0


t_host, ref = host_ms(host_load)
print(f"load {w}x{h} RGBA -> {p.W}x{p.H} (resized {p.rw}x{p.rh}): device {t_dev:.3f} ms, host torch {t_host:.1f} ms, "
      f"equal {torch.equal(out.cpu(), ref)}", flush=True)

# ---- to_uint8: 168 frames of 576 x 576
n = 168
rgb = torch.rand(n, 3, 576, 576, generator=g) * 2.2 - 1.1
x, u8 = rgb.to(dev), torch.empty(n, 576, 576, 3, dtype=torch.uint8, device=dev)
t_dev = device_ms(lambda: ops.rgb_to_u8(x, u8))
t_host, ref = host_ms(lambda: (((rgb.permute(0, 2, 3, 1) + 1) / 2.0) * 255).clamp(0, 255).to(torch.uint8))
gb = n * 576 * 576 * 15 / 1e9
print(f"to_uint8 {n} x 576x576: device {t_dev:.3f} ms ({gb / t_dev * 1e3:.0f} GB/s), host torch {t_host:.1f} ms, "
      f"equal {torch.equal(u8.cpu(), ref)}", flush=True)
