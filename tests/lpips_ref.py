"""LPIPS v0.1 with the VGG-16 backbone (Zhang et al. 2018; the `lpips` package's net="vgg", spatial=False, normalize=False) restated
in fp64 torch on UNROUNDED weights -- the reference of tests/test_lpips_cpu.py and tests/test_lpips_gpu.py -- with the inputs the two
share: synthetic name-keyed weights and three sizes of frame pairs.  Neither the `lpips` package nor its weights are installed:
this file is the published definition, not the package."""
import functools

import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)  # torchvision VGG-16 `features`: 3x3, pad 1, bias, ReLU
POOL_AFTER = (3, 8, 15, 22)                                # 2x2 / stride 2, floor, behind the ReLUs of convs 2, 7, 14, 21
TAPS = (2, 7, 14, 21, 28)                                  # ReLU outputs after these convs
WIDTHS = (64, 128, 256, 512, 512)

N = 3
CASES = ((40, 56), (32, 32), (64, 48))  # 40 x 56: pools 20x28, 10x14, 5x7, 2x3 (two odd floors); 32 x 32: the minimum, last tap 2x2
# The f16-operand floor per case: the error of the engine on the torch emulations of its operators (tests/fake_ops.py,
# tests/fake_lpips_ops.py: f16 operands, fp32 accumulation) against this file's fp64, worst absolute value over the frames of the
# five layer means and of their sum -- measured by tests/test_lpips_cpu.py, never by the code under test.  The GPU test's bound is
# twice this (the margin covers the MFMA accumulation order).
F16_FLOOR = {(40, 56): 4.862e-08, (32, 32): 1.818e-07, (64, 48): 5.819e-08}
LAYER_CS = (64, 128, 256, 512)
LAYER_HWS = (4, 35, 1120)  # one partial chunk; odd; five workgroups per pair (the slab sum runs)


def lpips_layers(sd: dict, a_u8: torch.Tensor, b_u8: torch.Tensor) -> torch.Tensor:
    """sd: fp32 state dict of `LpipsWeights`; a_u8, b_u8: uint8 (n,H,W,3) -> fp64 (n,5) layer means; LPIPS = .sum(1)."""
    shift = torch.tensor(SHIFT, dtype=torch.float64).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=torch.float64).view(1, 3, 1, 1)

    def taps(u8):
        x = (u8.permute(0, 3, 1, 2).double() / 127.5 - 1.0 - shift) / scale
        out = []
        for i in CONVS:
            x = F.relu(F.conv2d(x, sd[f"features.{i}.weight"].double(), sd[f"features.{i}.bias"].double(), padding=1))
            if i in TAPS:
                out.append(x)
            if i + 1 in POOL_AFTER:
                x = F.max_pool2d(x, 2, 2)
        return out

    res = []
    for k, (fa, fb) in enumerate(zip(taps(a_u8), taps(b_u8))):
        na = fa / (fa.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        nb = fb / (fb.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        w = sd[f"lin{k}.model.1.weight"].double().view(1, -1, 1, 1)
        res.append((w * (na - nb) ** 2).sum(1).mean(dim=(1, 2)))
    return torch.stack(res, 1)


def layer_sums_f64(fa: torch.Tensor, fb: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """The layer distance alone in fp64 on given features: f16 (n,hw,C) x 2, fp32 (C) -> fp64 (n) sums over the pixels."""
    a, b = fa.double(), fb.double()
    na = a / (a.pow(2).sum(2, keepdim=True).sqrt() + 1e-10)
    nb = b / (b.pow(2).sum(2, keepdim=True).sqrt() + 1e-10)
    return (w.double() * (na - nb) ** 2).sum(dim=(1, 2))


@functools.lru_cache(maxsize=None)
def state_dict(seed: int = 0) -> dict:
    """Synthetic weights under the public key names; do not modify (cached)."""
    from seva import metrics
    from seva import synthetic as synth
    return synth.synth_lpips_state_dict({k: tuple(v.shape) for k, v in metrics.LpipsWeights().state_dict().items()}, seed)


def weights(seed: int = 0):
    from seva import metrics
    w = metrics.LpipsWeights()
    w.load_state_dict(state_dict(seed), strict=True)
    return w


@functools.lru_cache(maxsize=None)
def pair(H: int, W: int, n: int = N):
    """-> (a, b) uint8 (n,H,W,3): a smooth pattern, and the same pattern shifted, dimmed and with +-12 noise; the LAST pair is
    identical.  Do not modify (cached)."""
    g = torch.Generator().manual_seed(4000 + 131 * H + W)
    y = torch.arange(H, dtype=torch.float64)[None, :, None, None]
    x = torch.arange(W, dtype=torch.float64)[None, None, :, None]
    c = torch.arange(3, dtype=torch.float64)[None, None, None, :]
    i = torch.arange(n, dtype=torch.float64)[:, None, None, None]
    a = 127.5 + 100.0 * torch.sin(0.31 * x + 0.7 * c + i) * torch.cos(0.23 * y - 0.4 * i)
    b = 120.0 + 90.0 * torch.sin(0.31 * x + 0.7 * c + i + 0.4) * torch.cos(0.23 * y - 0.4 * i) + \
        torch.randint(-12, 13, a.shape, generator=g)
    a, b = a.round().clamp(0, 255).to(torch.uint8), b.round().clamp(0, 255).to(torch.uint8)
    b[n - 1] = a[n - 1]
    return a, b


def to_f32(u8: torch.Tensor) -> torch.Tensor:
    """(n,H,W,3) uint8 -> (n,3,H,W) fp32 in [-1, 1] that the uint8 rule maps back to the same bytes (the interval centres)."""
    return ((u8.permute(0, 3, 1, 2).to(torch.float64) + 0.5) / 255.0 * 2.0 - 1.0).to(torch.float32).contiguous()


@functools.lru_cache(maxsize=None)
def reference(H: int, W: int) -> torch.Tensor:
    """fp64 (N,5) layer means of `pair(H, W)` under `state_dict()`, computed once."""
    return lpips_layers(state_dict(), *pair(H, W))


@functools.lru_cache(maxsize=None)
def layer_case(C: int, hw: int, n: int = N):
    """-> (fa, fb f16 (n,hw,C), w fp32 (C)): ReLU'd noise (half the features zero, as after a ReLU), fb = fa disturbed; cached."""
    g = torch.Generator().manual_seed(7000 + 13 * C + hw)
    fa = torch.randn((n, hw, C), generator=g).relu()
    fb = (fa + 0.3 * torch.randn((n, hw, C), generator=g)).relu()
    return fa.half(), fb.half(), (torch.randn(C, generator=g).abs() / C).contiguous()
