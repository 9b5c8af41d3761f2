"""Torch emulation of `ops.frame_metrics` for the CPU tests: the arithmetic contract of include/seva_hip.h
(`seva_frame_metrics`) restated operation by operation in fp32 -- separate multiplies and adds in the stated order, one
division -- so that the host logic of `seva.metrics` and `pipeline.run_scene(targets=...)` runs without a GPU and the
contract itself can be held against an fp64 SSIM."""
import torch

import fake_frame_ops

WIN = 11


def weights() -> torch.Tensor:
    """g[k] = exp(-(k-5)^2 / 4.5), normalised in fp64, rounded once to fp32."""
    k = torch.arange(WIN, dtype=torch.float64) - 5
    g = torch.exp(-(k * k) / 4.5)
    return (g / g.sum()).to(torch.float32)


def _pass(v: torch.Tensor, g: torch.Tensor, dim: int) -> torch.Tensor:
    """acc = 0; for k: acc = acc + g[k] * v[k], at valid positions along `dim`."""
    size = v.shape[dim] - (WIN - 1)
    acc = torch.zeros_like(v.narrow(dim, 0, size))
    for k in range(WIN):
        acc = acc + g[k] * v.narrow(dim, k, size)
    return acc


def ssim_map_f32(a_u8: torch.Tensor, b_u8: torch.Tensor) -> torch.Tensor:
    """(n,H,W,3) uint8 x 2 -> (n,3,H-10,W-10) fp32, the contract's expression."""
    g = weights()
    x = a_u8.permute(0, 3, 1, 2).to(torch.float32)
    y = b_u8.permute(0, 3, 1, 2).to(torch.float32)
    mx, my, exx, eyy, exy = (_pass(_pass(v, g, 3), g, 2) for v in (x, y, x * x, y * y, x * y))
    C1, C2 = torch.tensor(6.5025, dtype=torch.float32), torch.tensor(58.5225, dtype=torch.float32)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sx, sy, sxy = exx - mxx, eyy - myy, exy - mxy
    num = (2.0 * mxy + C1) * (2.0 * sxy + C2)
    den = ((mxx + myy) + C1) * ((sx + sy) + C2)
    return num / den


def frame_metrics(a, b, sse, ssim_sum=None, ssim_map=None, workspace=None):
    assert a.shape == b.shape and a.dtype == b.dtype
    ua, ub = fake_frame_ops.as_u8(a), fake_frame_ops.as_u8(b)
    d = ua.to(torch.int64) - ub.to(torch.int64)
    sse.copy_((d * d).sum(dim=(1, 2, 3)))
    if ssim_sum is None:
        assert ssim_map is None
        return
    H, W = ua.shape[1:3]
    if H < WIN or W < WIN:
        from seva._native import SevaNativeError
        raise SevaNativeError(f"frame_metrics: SSIM needs H, W >= 11 (the 11 x 11 window), got {H} x {W}")
    m = ssim_map_f32(ua, ub)
    ssim_sum.copy_(m.to(torch.float64).sum(dim=(1, 2, 3)))
    if ssim_map is not None:
        ssim_map.copy_(m)
