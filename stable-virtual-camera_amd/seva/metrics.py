"""Scores of generated frames against held-out pictures, on the device: PSNR, SSIM and LPIPS.

What the reference's evaluation tasks (`img2img`, `img2vid`) compute on the host from their saved samples, for the frames
this package produces:

    device  ONE call (`ops.frame_metrics`): per frame the exact squared error of the uint8 values and the sum of the SSIM map
            (Wang et al. 2004: 11 x 11 Gaussian window, sigma 1.5, valid positions, per channel; include/seva_hip.h)
    host    mse = sse / (3 H W), psnr = 10 log10(255^2 / mse), ssim = ssim_sum / (3 (H-10) (W-10)), in fp64

Both kinds of frames are scored on the same integers: uint8 (n,H,W,3) as `pipeline.run_scene` returns them, or fp32
(n,3,H,W) in [-1, 1] as `AutoEncoder.decode` returns them, taken through `frames.to_uint8`'s rule as they are loaded.
There is no CPU fallback: tensors that are not on an AMD GPU raise `SevaNativeError`.

LPIPS v0.1 with the VGG-16 backbone (Zhang et al. 2018; the `lpips` package's `net="vgg"`, `spatial=False`,
`normalize=False`) runs on the same integers: the tower's input is `u8 / 127.5 - 1`, through the scaling layer
`(x - shift) / scale`, the 13 convolutions of torchvision's VGG-16 `features` on `ops.conv3x3`, and per tap (the ReLU outputs
after convs 2, 7, 14, 21, 28) the unit-normalised, linearly weighted squared difference averaged over the pixels
(`seva/_lpips_engine.py`, csrc/lpips.hip).  The network is pretrained and its weights are not part of this package:
`LpipsWeights` holds them under the key names below and `load_lpips_weights` reads them from local files; nothing is fetched.
The key names (`features.{i}.weight` / `.bias` of torchvision's VGG-16, `lin{k}.model.1.weight` and the `net.slice{j}.{i}.`
prefix of the `lpips` package) are taken from the two packages' public source and are NOT checked against them here, because
neither package is installed: parity with the `lpips` package is unpinned, the tests hold the HIP path against a torch
restatement of the published definition (tests/lpips_ref.py) on synthetic weights.
"""

from __future__ import annotations

import os
import re

import torch
from torch import nn

from . import ops
from ._lpips_engine import VGG_WIDTHS, conv_shapes

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


def compare(a: torch.Tensor, b: torch.Tensor, *, ssim: bool = True, ssim_map: bool = False, lpips: "LPIPS | None" = None) -> dict:
    """Per-frame scores of `a` against `b`: {"sse": int64 (n), "mse", "psnr", ["ssim"]: fp64 (n), ["ssim_map"]: fp32
    (n,3,H-10,W-10)} on the frames' device.  psnr = 10 log10(255^2 3HW / sse), inf where the frames are equal.
    `ssim=False` computes the squared error only (no size limit); SSIM needs H, W >= 11.
    `lpips` (an `LPIPS` on the frames' device) adds "lpips": fp64 (n) and "lpips_layers": fp64 (n,5); H, W >= 32."""
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
    if lpips is not None:
        out["lpips_layers"] = lpips.layers(a, b)
        out["lpips"] = out["lpips_layers"].sum(1)
    return out


def psnr(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """fp64 (n): PSNR in dB of the uint8 frames, inf for equal frames."""
    return compare(a, b, ssim=False)["psnr"]


def ssim(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """fp64 (n): mean SSIM over channels and valid positions."""
    return compare(a, b)["ssim"]


# ---- LPIPS -----------------------------------------------------------------------------------------------------------------
class _Conv(nn.Module):
    """Parameter holder of one convolution (the engine packs the weights; nothing here computes)."""

    def __init__(self, cout: int, cin: int, k: int, bias: bool):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(cout, cin, k, k), requires_grad=False)
        if bias:
            self.bias = nn.Parameter(torch.zeros(cout), requires_grad=False)


class _Lin(nn.Module):
    def __init__(self, c: int):
        super().__init__()
        self.model = nn.ModuleDict({"1": _Conv(1, c, 1, False)})  # (index 0 of the package's Sequential is a Dropout)


class LpipsWeights(nn.Module):
    """The pretrained parameters of LPIPS v0.1 / VGG-16 under their public names: `features.{i}.weight` (cout,cin,3,3) and
    `features.{i}.bias` for i in 0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28 (torchvision's VGG-16), and
    `lin{k}.model.1.weight` (1,C,1,1), C = 64, 128, 256, 512, 512 (the `lpips` package's linear layers, >= 0).  Loading is strict."""

    def __init__(self):
        super().__init__()
        self.features = nn.ModuleDict({str(i): _Conv(co, ci, 3, True) for i, (co, ci) in conv_shapes().items()})
        for k, c in enumerate(VGG_WIDTHS):
            setattr(self, f"lin{k}", _Lin(c))

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        return super().load_state_dict(_canonical_lpips_keys(state_dict), strict=strict, **kw)


_SLICE_KEY = re.compile(r"^net\.slice\d+\.(\d+)\.(weight|bias)$")


def _canonical_lpips_keys(sd: dict) -> dict:
    """`net.slice{j}.{i}.x` -> `features.{i}.x` (the `lpips` package keeps torchvision's layer indices inside its slices); the
    package's `scaling_layer.*` buffers (this library's constants) and torchvision's `classifier.*` are dropped."""
    out = {}
    for k, v in sd.items():
        m = _SLICE_KEY.match(k)
        k = f"features.{m.group(1)}.{m.group(2)}" if m else k
        if k.startswith(("scaling_layer.", "classifier.")):
            continue
        if k in out:
            raise ValueError(f"LPIPS weights: {k} given twice (as features.* and as net.slice*.*)")
        out[k] = v
    return out


def load_lpips_weights(path: str | None = None, lin_path: str | None = None) -> LpipsWeights:
    """`LpipsWeights` from LOCAL files (nothing is fetched): `path` is one merged state dict (every key of `LpipsWeights`, the
    `net.slice{j}.{i}.` prefix accepted), or -- with `lin_path` -- a torchvision VGG-16 state dict (`features.*`; its
    `classifier.*` is ignored) beside the `lpips` package's linear-layer file (`lin{k}.model.1.weight`).  Arguments not given
    come from SEVA_LPIPS_VGG_PATH and SEVA_LPIPS_LIN_PATH.  Strict: a missing, unexpected or misshapen key is an error."""
    path = path or os.environ.get("SEVA_LPIPS_VGG_PATH")
    lin_path = lin_path or os.environ.get("SEVA_LPIPS_LIN_PATH")
    if not path:
        raise ValueError("LPIPS weights: give a local file (path=, or SEVA_LPIPS_VGG_PATH); nothing is downloaded")
    sd = dict(torch.load(path, map_location="cpu", weights_only=True))
    if lin_path:
        lin = torch.load(lin_path, map_location="cpu", weights_only=True)
        both = sorted(set(_canonical_lpips_keys(sd)) & set(_canonical_lpips_keys(lin)))
        if both:
            raise ValueError(f"LPIPS weights: {both[:3]} are in both files")
        sd.update(lin)
    w = LpipsWeights()
    w.load_state_dict(sd, strict=True)
    return w


class LPIPS(nn.Module):
    """LPIPS v0.1 / VGG-16 on the HIP kernels: `m = LPIPS(weights).to("cuda")`; `m(a, b)` -> fp64 (n), `m.layers(a, b)` -> fp64
    (n,5), for frames as `compare` takes them (H, W >= 32).  `chunk_size`: pairs per pass (default: what keeps the activations
    of a pass below 4 GiB); a pair's score does not depend on it.  No CPU fallback."""

    def __init__(self, weights: LpipsWeights, chunk_size: int | None = None):
        super().__init__()
        self.weights = weights
        self.chunk_size = chunk_size
        self._engine = None

    def _apply(self, fn, *a, **k):
        self._engine = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._engine = None
        return super().load_state_dict(*a, **k)

    def engine(self):
        if self._engine is None:
            from ._lpips_engine import LpipsEngine
            self._engine = LpipsEngine(self.weights, chunk_size=self.chunk_size)
        return self._engine

    def layers(self, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        _kind(a, b)
        return self.engine().layers(_dense(a), _dense(b))

    def forward(self, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        return self.layers(a, b).sum(1)
