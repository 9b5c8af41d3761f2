"""Image-space scores of generated frames against held-out pictures, on the device: PSNR and SSIM.

What the reference's evaluation tasks (`img2img`, `img2vid`) compute on the host from their saved samples, for the frames
this package produces:

    device  ONE call (`ops.frame_metrics`): per frame the exact squared error of the uint8 values and the sum of the SSIM map
            (Wang et al. 2004: 11 x 11 Gaussian window, sigma 1.5, valid positions, per channel; include/seva_hip.h)
    host    mse = sse / (3 H W), psnr = 10 log10(255^2 / mse), ssim = ssim_sum / (3 (H-10) (W-10)), in fp64

Both kinds of frames are scored on the same integers: uint8 (n,H,W,3) as `pipeline.run_scene` returns them, or fp32
(n,3,H,W) in [-1, 1] as `AutoEncoder.decode` returns them, taken through `frames.to_uint8`'s rule as they are loaded.
There is no CPU fallback: tensors that are not on an AMD GPU raise `SevaNativeError`.  Not ported: LPIPS (it needs a
pretrained network).
"""

from __future__ import annotations

import torch

from . import ops

WINDOW = 11  # SSIM window; H, W >= WINDOW


def _kind(a: torch.Tensor, b: torch.Tensor) -> tuple[int, int, int]:
    if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)):
        raise ValueError("a, b: tensors")
    if a.dtype != b.dtype or a.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"a, b: both uint8 (n,H,W,3) or both float32 (n,3,H,W); got {a.dtype}, {b.dtype}")
    if a.dim() != 4 or a.shape != b.shape:
        raise ValueError(f"a, b: the same 4-d shape; got {tuple(a.shape)}, {tuple(b.shape)}")
    if a.device != b.device:
        raise ValueError(f"a, b: the same device; got {a.device}, {b.device}")
    if a.dtype == torch.uint8:
        n, H, W, c = a.shape
    else:
        n, c, H, W = a.shape
    if c != 3 or n < 1 or H < 1 or W < 1:
        raise ValueError(f"a, b: uint8 (n,H,W,3) or float32 (n,3,H,W) with n, H, W >= 1; got {tuple(a.shape)}")
    return n, H, W


def _dense(x: torch.Tensor) -> torch.Tensor:
    """Images dense inside (any pitch between them), as the kernel reads them."""
    return x if x[0].is_contiguous() else x.contiguous()


def compare(a: torch.Tensor, b: torch.Tensor, *, ssim: bool = True, ssim_map: bool = False) -> dict:
    """Per-frame scores of `a` against `b`: {"sse": int64 (n), "mse", "psnr", ["ssim"]: fp64 (n), ["ssim_map"]: fp32
    (n,3,H-10,W-10)} on the frames' device.  psnr = 10 log10(255^2 3HW / sse), inf where the frames are equal.
    `ssim=False` computes the squared error only (no size limit); SSIM needs H, W >= 11."""
    n, H, W = _kind(a, b)
    if ssim_map and not ssim:
        raise ValueError("ssim_map=True needs ssim=True")
    a, b = _dense(a), _dense(b)
    dev = a.device
    sse = torch.empty(n, dtype=torch.int64, device=dev)
    ssum = torch.empty(n, dtype=torch.float64, device=dev) if ssim else None
    smap = torch.empty((n, 3, H - (WINDOW - 1), W - (WINDOW - 1)), dtype=torch.float32, device=dev) \
        if (ssim_map and H >= WINDOW and W >= WINDOW) else None
    ops.frame_metrics(a, b, sse, ssum, smap)
    elems = 3 * H * W
    s = sse.to(torch.float64)
    out = {"sse": sse, "mse": s / elems}
    out["psnr"] = torch.where(sse == 0, torch.full_like(s, float("inf")),
                              10.0 * torch.log10((255.0 ** 2 * elems) / s.clamp_min(1.0)))
    if ssim:
        out["ssim"] = ssum / float(3 * (H - (WINDOW - 1)) * (W - (WINDOW - 1)))
    if ssim_map:
        out["ssim_map"] = smap
    return out


def psnr(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """fp64 (n): PSNR in dB of the uint8 frames, inf for equal frames."""
    return compare(a, b, ssim=False)["psnr"]


def ssim(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """fp64 (n): mean SSIM over channels and valid positions."""
    return compare(a, b)["ssim"]
