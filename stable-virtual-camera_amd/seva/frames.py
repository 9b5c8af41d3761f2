"""Image front and back end of the pipeline on the device: pictures + intrinsics -> [-1, 1] frames, frames -> uint8.

What the reference does on the CPU in torch (seva/eval.py: `load_img_and_K` 160-246, `transform_img_and_K` 249-322 and the
`(v + 1) / 2 * 255 -> uint8` rule of `save_output` 974-975), for callers of this package's own `pipeline`:

    host    `plan_load` / `plan_transform`: the integer geometry (resized size, crop or pad window, output size) with the
            reference's rounding; `adjust_K`: the matching change of the intrinsics
    device  ONE kernel per call (`ops.image_area_crop`): uint8 -> float, alpha compositing, area resize, crop / pad and the
            `* 2 - 1` map, computing only the output pixels, bit for bit the reference's fp32 arithmetic;
            `ops.rgb_to_u8` for the way back

The source bytes go to the device as uint8; nothing image-sized is touched by torch arithmetic.  There is no CPU
fallback: tensors that are not on an AMD GPU raise `SevaNativeError` like every other operator.  Not ported: PIL output
(`image_as_tensor=False`), video and PNG writing.
"""

from __future__ import annotations

import math
import os
from typing import NamedTuple, Sequence

import numpy as np
import torch

from . import ops


class FramePlan(NamedTuple):
    """Geometry of one load / transform.  The source is area-resized to (rh, rw); the reference then pads by (pt, pl)
    at the top / left and crops at (ct, cl) of the padded image, so the (H, W) output window starts at
    (ct - pt, cl - pl) of the resized image."""
    rh: int
    rw: int
    ct: int
    cl: int
    pl: int
    pt: int
    H: int
    W: int


def get_resizing_factor(target_shape: Sequence[int], current_shape: Sequence[int], cover_target: bool = True) -> float:
    """Scale from `current_shape` (H, W) at which the image just covers (`cover_target`) or just fits inside the target
    (H, W) (eval.py:99-138)."""
    t_lo, t_hi = min(target_shape), max(target_shape)
    c_lo, c_hi = min(current_shape), max(current_shape)
    bound = target_shape[1] / target_shape[0]
    aspect = current_shape[1] / current_shape[0]
    if bound >= 1.0:
        beyond, opposite = aspect >= bound, aspect < 1.0
    else:
        beyond, opposite = aspect <= bound, aspect > 1.0
    if cover_target:
        num, den = (t_lo, c_lo) if beyond else (t_hi, c_lo) if opposite else (t_hi, c_hi)
    else:
        num, den = (t_hi, c_hi) if beyond else (t_lo, c_hi) if opposite else (t_lo, c_lo)
    return num / den


def get_wh_with_fixed_shortest_side(w: int, h: int, size: int | None) -> tuple[int, int]:
    """(w, h) with the shorter side at `size`, the other truncated; None or <= 0 keeps the size (eval.py:147-157)."""
    if size is None or size <= 0:
        return w, h
    if w < h:
        return size, int(size * h / w)
    return int(size * w / h), size


def _target_wh(w, h, size, size_stride):
    W, H = size if isinstance(size, (tuple, list)) else get_wh_with_fixed_shortest_side(w, h, size)
    return math.floor(W / size_stride + 0.5) * size_stride, math.floor(H / size_stride + 0.5) * size_stride


def _clamped_origin(centre: int, length: int, extent: int) -> int:
    return min(max(0, centre - length // 2), extent - length)


def plan_load(h: int, w: int, size, scale: float = 1.0, center=(0.5, 0.5), size_stride: int = 1,
              center_crop: bool = False) -> FramePlan:
    """Geometry of `load_img_and_K` for an (h, w) source (eval.py:192-229).  `size`: (W, H) to cover and crop, an int for
    the shorter side, None for the source size.  `scale` < 1 shrinks the picture inside a white (W, H) canvas."""
    W, H = _target_wh(w, h, (w, h) if size is None else size, size_stride)
    f = get_resizing_factor((math.floor(H * scale), math.floor(W * scale)), (h, w))
    rh, rw = math.ceil(f * h), math.ceil(f * w)
    pt = pl = 0
    if scale < 1.0:
        pl, pt = math.ceil((W - rw) * 0.5), math.ceil((H - rh) * 0.5)
    ih, iw = rh + 2 * pt, rw + 2 * pl  # the padded image the crop is taken from
    oh, ow = (min(H, W),) * 2 if center_crop else (H, W)
    ct = _clamped_origin(int(center[1] * ih), oh, ih)
    cl = _clamped_origin(int(center[0] * iw), ow, iw)
    return FramePlan(rh, rw, ct, cl, pl, pt, oh, ow)


def plan_transform(h: int, w: int, size, scale: float = 1.0, center=(0.5, 0.5), size_stride: int = 1,
                   mode: str = "crop") -> FramePlan:
    """Geometry of `transform_img_and_K` (eval.py:264-311).  `crop`: cover (W, H), then crop; `pad`: fit inside, then
    zero-pad; `stretch`: resize to (W, H) ignoring the aspect ratio.  `scale` divides the resized size."""
    if mode not in ("crop", "pad", "stretch"):
        raise ValueError(f"mode should be one of ['crop', 'pad', 'stretch'], got {mode}")
    W, H = _target_wh(w, h, size, size_stride)
    if mode == "stretch":
        rh, rw = H, W
    else:
        f = get_resizing_factor((H, W), (h, w), cover_target=mode != "pad")
        rh, rw = math.ceil(f * h), math.ceil(f * w)
    rh, rw = int(rh / scale), int(rw / scale)
    cy, cx = int(center[1] * rh), int(center[0] * rw)
    if mode != "pad":
        return FramePlan(rh, rw, _clamped_origin(cy, H, rh), _clamped_origin(cx, W, rw), 0, 0, H, W)
    pt, pl = max(0, H // 2 - cy), max(0, W // 2 - cx)
    pb, pr = max(0, H - pt - rh), max(0, W - pl - rw)
    return FramePlan(rh, rw, 0, 0, pl, pt, pt + rh + pb, pl + rw + pr)


def adjust_K(K: torch.Tensor, plan: FramePlan, h: int, w: int, *, shift=None) -> torch.Tensor:
    """Intrinsics after the resize and the crop (eval.py:231-237, 313-320): (3, 3) or (n, 3, 3).  A K whose principal point
    lies in [0, 1]^2 (over the whole batch) is taken as normalised and scaled by the resized size, any other as pixels of
    the (h, w) source and scaled by resized / source.  `shift` = (dx, dy) added to the principal point, default
    (pl - cl, pt - ct)."""
    K = K.clone()
    pp = K[..., :2, -1]
    if torch.all(pp >= 0) and torch.all(pp <= 1):
        K[..., :2, :] *= K.new_tensor([plan.rw, plan.rh])[:, None]
    else:
        K[..., :2, :] *= K.new_tensor([plan.rw / w, plan.rh / h])[:, None]
    dx, dy = (plan.pl - plan.cl, plan.pt - plan.ct) if shift is None else shift
    K[..., :2, 2] += K.new_tensor([dx, dy])
    return K


def _source_u8(image, device) -> torch.Tensor:
    """-> uint8 (1, h, w, 3 | 4) on `device`; the bytes travel as they are."""
    if isinstance(image, torch.Size):
        h, w = image
        return torch.zeros((1, h, w, 4), dtype=torch.uint8, device=device)  # Image.new("RGBA", (w, h)): transparent black
    if isinstance(image, (str, os.PathLike)):
        from PIL import Image
        with Image.open(image) as im:
            image = np.array(im.convert("RGBA"))
    if isinstance(image, np.ndarray):
        image = torch.from_numpy(np.ascontiguousarray(image))
    if not (isinstance(image, torch.Tensor) and image.dtype == torch.uint8 and image.dim() == 3 and image.shape[-1] in (3, 4)):
        raise ValueError("image: a path, a torch.Size (h, w) or a uint8 (h, w, 3 | 4) array / tensor")
    return image.to(device).contiguous()[None]


def load_img_and_K(image_path_or_size_or_uint8_array, size, scale: float = 1.0, center=(0.5, 0.5),
                   K: torch.Tensor | None = None, size_stride: int = 1, center_crop: bool = False,
                   image_as_tensor: bool = True, context_rgb=None, device="cuda"):
    """The reference's `load_img_and_K` with the image work in one kernel: -> ((1, 3, H, W) fp32 in [-1, 1] on `device`,
    adjusted K or None).  The source is a PNG / JPEG path (read through PIL), a `torch.Size` (h, w) meaning a blank RGBA
    picture, or a uint8 (h, w, 3 | 4) array or tensor.  `context_rgb`: (h, w, 3) float background behind the alpha
    channel (default white).  As in the reference, K's principal point moves by the crop origin only."""
    if not image_as_tensor:
        raise ValueError("image_as_tensor=False (PIL output) is the reference's CPU path; this module returns device tensors")
    device = torch.device(device)
    src = _source_u8(image_path_or_size_or_uint8_array, device)
    h, w = src.shape[1:3]
    p = plan_load(h, w, size, scale, center, size_stride, center_crop)
    ctx = None
    if context_rgb is not None:
        if src.shape[-1] != 4:
            raise ValueError("context_rgb needs a source with an alpha channel")
        ctx = torch.as_tensor(context_rgb).to(device=device, dtype=torch.float32).contiguous()
    out = torch.empty((1, 3, p.H, p.W), dtype=torch.float32, device=device)
    ops.image_area_crop(src, out, rh=p.rh, rw=p.rw, ct=p.ct - p.pt, cl=p.cl - p.pl, pad_value=1.0, out_mul=2.0, out_add=-1.0,
                        context_rgb=ctx)
    return out, (None if K is None else adjust_K(K, p, h, w, shift=(-p.cl, -p.ct)))


def transform_img_and_K(image: torch.Tensor, size, scale: float = 1.0, center=(0.5, 0.5), K: torch.Tensor | None = None,
                        size_stride: int = 1, mode: str = "crop"):
    """The reference's `transform_img_and_K`: image (n, 3, h, w) fp32 on the device, K (n, 3, 3) or None ->
    ((n, 3, H', W'), K).  Where the window leaves the resized image (`pad`, or a crop larger than it) the pixels are 0."""
    if image.dim() != 4 or image.shape[1] != 3 or image.dtype != torch.float32:
        raise ValueError("image: (n, 3, h, w) float32")
    n, _, h, w = image.shape
    p = plan_transform(h, w, size, scale, center, size_stride, mode)
    if image.stride(3) != 1:
        image = image.contiguous()
    out = torch.empty((n, 3, p.H, p.W), dtype=torch.float32, device=image.device)
    ops.image_area_crop(image, out, rh=p.rh, rw=p.rw, ct=p.ct - p.pt, cl=p.cl - p.pl)
    return out, (None if K is None else adjust_K(K, p, h, w))


def to_uint8(rgb: torch.Tensor) -> torch.Tensor:
    """(n, 3, H, W) fp32 in [-1, 1] -> (n, H, W, 3) uint8, `save_output`'s rule: (v + 1) / 2 * 255, clamped, truncated.
    NaN -> 0 (the reference leaves it undefined)."""
    if rgb.dim() != 4 or rgb.shape[1] != 3 or rgb.dtype != torch.float32:
        raise ValueError("rgb: (n, 3, H, W) float32")
    n, _, H, W = rgb.shape
    if not (rgb.stride(3) == 1 and rgb.stride(2) == W and rgb.stride(1) == H * W):
        rgb = rgb.contiguous()
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=rgb.device)
    ops.rgb_to_u8(rgb, out)
    return out
