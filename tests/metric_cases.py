"""Inputs and the fp64 reference shared by tests/test_metrics_cpu.py and tests/test_metrics_gpu.py: six pairs of uint8
frame batches at n = 3, 37 x 53 (more than one 32 x 32 tile each way, neither side a multiple of the tile, 159-byte rows)
and noise pairs at three more sizes; SSE in int64 and the SSIM of Wang et al. 2004 in fp64 (`conv2d`, valid padding)."""
import functools

import torch
import torch.nn.functional as F

N, H0, W0 = 3, 37, 53
PAIRS = ("noise", "smooth_pm6", "white_one_254", "white_black", "identical", "white_half_black")
SIZES = ((11, 11), (12, 43), (64, 96))  # one valid position; one valid row; tile-exact
FRAME_TOL, MAP_TOL = 1e-5, 1e-3          # a score quoted to four decimals must not move; maps are for looking at


def _noise(g, n, H, W):
    return torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.int64).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def pair(name: str, H: int = H0, W: int = W0, n: int = N):
    """-> (a, b) uint8 (n,H,W,3) on the CPU; do not modify (cached)."""
    g = torch.Generator().manual_seed(1000 + 7 * PAIRS.index(name) + H * 131 + W)
    white = torch.full((n, H, W, 3), 255, dtype=torch.uint8)
    if name == "noise":
        return _noise(g, n, H, W), _noise(g, n, H, W)
    if name == "smooth_pm6":
        y = torch.arange(H, dtype=torch.float64)[None, :, None, None]
        x = torch.arange(W, dtype=torch.float64)[None, None, :, None]
        c = torch.arange(3, dtype=torch.float64)[None, None, None, :]
        i = torch.arange(n, dtype=torch.float64)[:, None, None, None]
        a = (127.5 + 100.0 * torch.sin(0.21 * x + 0.5 * c + i) * torch.cos(0.17 * y - 0.3 * i)).round().to(torch.int64)
        b = (a + torch.randint(-6, 7, a.shape, generator=g)).clamp(0, 255)
        return a.to(torch.uint8), b.to(torch.uint8)
    if name == "white_one_254":
        b = white.clone()
        for i, (yy, xx, cc) in enumerate(((H // 2, W // 2, 1), (0, 0, 0), (H - 1, W - 1, 2))[:n]):
            b[i, yy, xx, cc] = 254
        return white, b
    if name == "white_black":
        return white, torch.zeros_like(white)
    if name == "identical":
        a = _noise(g, n, H, W)
        return a, a.clone()
    if name == "white_half_black":
        b = white.clone()
        b[0, :, : W // 2] = 0
        if n > 1:
            b[1, H // 2:] = 0
        if n > 2:
            b[2, :, W // 2:, 1] = 0
        return white, b
    raise KeyError(name)


def all_cases():
    """[(id, a, b)]: the six pairs at 37 x 53, then noise at the three other sizes."""
    out = [(p, *pair(p)) for p in PAIRS]
    out += [(f"noise_{h}x{w}", *pair("noise", h, w)) for h, w in SIZES]
    return out


def to_f32(u8: torch.Tensor) -> torch.Tensor:
    """(n,H,W,3) uint8 -> (n,3,H,W) fp32 in [-1, 1] that the uint8 rule ((v + 1) / 2 * 255, truncated) maps back to the same
    bytes: the centre of each byte's interval."""
    return ((u8.permute(0, 3, 1, 2).to(torch.float64) + 0.5) / 255.0 * 2.0 - 1.0).to(torch.float32).contiguous()


def sse_i64(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    d = a.to(torch.int64) - b.to(torch.int64)
    return (d * d).sum(dim=(1, 2, 3))


def ssim_map_f64(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """(n,H,W,3) uint8 x 2 -> (n,3,H-10,W-10) fp64."""
    k = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-(k * k) / 4.5)
    g = g / g.sum()
    w = torch.outer(g, g)[None, None].repeat(3, 1, 1, 1)
    x = a.permute(0, 3, 1, 2).to(torch.float64)
    y = b.permute(0, 3, 1, 2).to(torch.float64)

    def blur(v):
        return F.conv2d(v, w, groups=3)

    mx, my = blur(x), blur(y)
    sx, sy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    return ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sx + sy + C2))


@functools.lru_cache(maxsize=None)
def reference(case_id: str):
    """-> (sse int64 (n), ssim fp64 (n), map fp64) of one case of `all_cases`, computed once."""
    a, b = next((a, b) for cid, a, b in all_cases() if cid == case_id)
    m = ssim_map_f64(a, b)
    return sse_i64(a, b), m.mean(dim=(1, 2, 3)), m
