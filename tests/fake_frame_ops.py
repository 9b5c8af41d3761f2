"""Torch emulation of the two frame kernels (`ops.image_area_crop`, `ops.rgb_to_u8`) for the CPU tests: the arithmetic
contract of include/seva_hip.h restated with plain fp32 torch operations, one rounding per operation, in the stated order.
It does NOT call F.interpolate: that it reproduces the reference's images bit for bit is what pins the contract."""
import torch


def _windows(size_in: int, size_out: int):
    i = torch.arange(size_out, dtype=torch.int64)
    lo = (i * size_in) // size_out
    hi = ((i + 1) * size_in + size_out - 1) // size_out
    return lo, hi - lo


def _area(x: torch.Tensor, rh: int, rw: int) -> torch.Tensor:
    """x (n,3,h,w) fp32 -> (n,3,rh,rw): window sums in row-major order starting from 0, / rows, / columns."""
    h, w = x.shape[-2:]
    y0, kh = _windows(h, rh)
    x0, kw = _windows(w, rw)
    s = torch.zeros(x.shape[:2] + (rh, rw), dtype=torch.float32)
    for dy in range(int(kh.max())):
        rows = x[:, :, (y0 + dy).clamp(max=h - 1)]
        for dx in range(int(kw.max())):
            v = rows[:, :, :, (x0 + dx).clamp(max=w - 1)]
            inside = (dy < kh)[:, None] & (dx < kw)[None, :]
            s = torch.where(inside, s + v, s)
    return s / kh[:, None].float() / kw[None, :].float()


def image_area_crop(src, out, *, rh, rw, ct=0, cl=0, pad_value=0.0, out_mul=1.0, out_add=0.0, context_rgb=None):
    n, _, H, W = out.shape
    if src.dtype == torch.uint8:
        v = src.permute(0, 3, 1, 2).float() / 255.0
        if v.shape[1] == 4:
            rgb, a = v[:, :3], v[:, 3:]
            bg = torch.ones(()) if context_rgb is None else context_rgb.permute(2, 0, 1)[None]
            v = rgb * a + bg * (1.0 - a)
        else:
            assert context_rgb is None
    else:
        assert src.dtype == torch.float32 and context_rgb is None
        v = src
    r = _area(v.contiguous(), rh, rw)
    res = torch.full((n, 3, H, W), float(pad_value), dtype=torch.float32)
    ys, xs = torch.arange(H) + ct, torch.arange(W) + cl
    oky, okx = (ys >= 0) & (ys < rh), (xs >= 0) & (xs < rw)
    inside = oky[:, None] & okx[None, :]
    res[:, :, inside] = r[:, :, ys[oky]][:, :, :, xs[okx]].reshape(n, 3, -1)
    if not (float(out_mul) == 1.0 and float(out_add) == 0.0):
        res = res * float(out_mul) + float(out_add)
    out.copy_(res)


def rgb_to_u8(x, out):
    t = (x + 1.0) / 2.0
    t = (t * 255.0).clamp(0, 255)
    t = torch.where(torch.isnan(t), torch.zeros(()), t)
    out.copy_(t.permute(0, 2, 3, 1).to(torch.uint8))


def as_u8(x: torch.Tensor) -> torch.Tensor:
    """(n,H,W,3) uint8 of a frame batch of either kind: uint8 NHWC as it is, fp32 NCHW through the uint8 rule."""
    if x.dtype == torch.uint8:
        return x
    out = torch.empty((x.shape[0], x.shape[2], x.shape[3], 3), dtype=torch.uint8)
    rgb_to_u8(x, out)
    return out
