"""Device time of the frame scores (`metrics.compare`: squared error + SSIM of 168 frames of 576 x 576, both input kinds) beside
the same expression in torch on the host (no threshold: scoring is not on the sampler's critical path; DESIGN.md quotes it).
Run from the repository root on an MI355X:  python tools/kmetrics_time.py"""
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, "stable-virtual-camera_amd")
from seva import frames, metrics, ops  # noqa: E402

dev = torch.device("cuda:0")
torch.set_num_threads(min(16, torch.get_num_threads()))
g = torch.Generator().manual_seed(0)
n, H, W = 168, 576, 576


def device_ms(fn):
    fn()  # warm-up: code object load, allocator
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def host_scores(a, b):
    """The same scores in fp32 torch on the host: (n,H,W,3) uint8 x 2 -> (sse, ssim)."""
    k = torch.arange(11, dtype=torch.float64) - 5
    gk = torch.exp(-(k * k) / 4.5)
    gk = (gk / gk.sum()).float()
    wy, wx = gk.view(1, 1, 11, 1).repeat(3, 1, 1, 1), gk.view(1, 1, 1, 11).repeat(3, 1, 1, 1)
    sse, ssim = [], []
    for i in range(a.shape[0]):  # frame by frame: five 576 x 576 x 3 planes at a time
        d = a[i].to(torch.int64) - b[i].to(torch.int64)
        sse.append((d * d).sum())
        x, y = a[i].permute(2, 0, 1)[None].float(), b[i].permute(2, 0, 1)[None].float()
        mx, my, exx, eyy, exy = (F.conv2d(F.conv2d(v, wx, groups=3), wy, groups=3) for v in (x, y, x * x, y * y, x * y))
        sx, sy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
        m = ((2 * mx * my + 6.5025) * (2 * sxy + 58.5225)) / ((mx * mx + my * my + 6.5025) * (sx + sy + 58.5225))
        ssim.append(m.double().mean())
    return torch.stack(sse), torch.stack(ssim)


rgb_a = torch.rand(n, 3, H, W, generator=g) * 2.2 - 1.1
rgb_b = (rgb_a + 0.05 * torch.randn(n, 3, H, W, generator=g)).contiguous()
fa, fb = rgb_a.to(dev), rgb_b.to(dev)
ua, ub = frames.to_uint8(fa), frames.to_uint8(fb)
sse = torch.empty(n, dtype=torch.int64, device=dev)
ssum = torch.empty(n, dtype=torch.float64, device=dev)
ws = torch.empty(ops.frame_metrics_workspace_numel(n, H, W), dtype=torch.uint8, device=dev)

t_u8 = device_ms(lambda: ops.frame_metrics(ua, ub, sse, ssum, None, ws))
got_u8 = (sse.clone(), ssum.clone())
t_f32 = device_ms(lambda: ops.frame_metrics(fa, fb, sse, ssum, None, ws))
same = torch.equal(sse, got_u8[0]) and torch.equal(ssum, got_u8[1])
t_sse = device_ms(lambda: ops.frame_metrics(ua, ub, sse, None, None, ws))
m = metrics.compare(ua, ub)
t = time.perf_counter()
ref_sse, ref_ssim = host_scores(ua.cpu(), ub.cpu())
t_host = (time.perf_counter() - t) * 1e3
gb_u8, gb_f32 = n * H * W * 3 * 2 / 1e9, n * H * W * 3 * 8 / 1e9
print(f"scores of {n} x {W}x{H} frames (squared error + SSIM): uint8 frames {t_u8:.3f} ms ({gb_u8 / t_u8 * 1e3:.0f} GB/s read), "
      f"fp32 frames {t_f32:.3f} ms ({gb_f32 / t_f32 * 1e3:.0f} GB/s read), both kinds bit-equal {same}; squared error only "
      f"{t_sse:.3f} ms; host torch (fp32, {torch.get_num_threads()} threads) {t_host:.0f} ms", flush=True)
print(f"  sse equal to the host's {torch.equal(m['sse'].cpu(), ref_sse)}, worst |ssim - host fp32| "
      f"{float((m['ssim'].cpu() - ref_ssim).abs().max()):.2e}; psnr {float(m['psnr'].min()):.2f} .. {float(m['psnr'].max()):.2f} dB, "
      f"ssim {float(m['ssim'].min()):.4f} .. {float(m['ssim'].max()):.4f}", flush=True)
