"""HIP execution of LPIPS v0.1 with the VGG-16 backbone (Zhang et al. 2018; `seva.metrics.LPIPS`).  Same rules as the VAE engine:
channels-last f16 activations, every convolution on `ops.conv3x3` (implicit GEMM, fp32 accumulation, bias in the epilogue, one
rounding to f16), and three operators of its own around them (csrc/lpips.hip; the contract is in include/seva_hip.h):

  prepare     ops.lpips_prepare: frames of either kind -> the scaling layer's output as the 64-channel padded first-conv operand
  conv x13    ops.conv3x3(..., out_f16=raw) | ops.lpips_relu_pool(raw, raw[, pooled]): ReLU in place -- the tap and the next conv's
              operand -- and after convs 3, 8, 15, 22 the 2 x 2 max-pool into the next level's operand
  tap x5      ops.lpips_layer: per pair the sum over pixels of sum_c w[c] (a_c / |a| - b_c / |b|)^2, fp64; the host divides by h w

The two frames of a pair run as ONE batch of 2m frames per chunk (a in the first half, b in the second): every conv sees both,
and a tap's two operands are the two halves of one tensor.  A chunk is `chunk_size` pairs; the arena holds one chunk's
activations (three full-resolution 64-channel tensors dominate: 576 x 576 x 64 f16 is 42 MB per frame, 168 pairs at once would be
7 GB per tensor), so the default chunk is what keeps it below ARENA_BYTES.  A pair's result does not depend on its chunk.
"""

from __future__ import annotations

import torch

from . import ops
from ._engine import CIN_PAD, _EngineBase, pack_conv3x3
from ._native import require_cuda

F16, F32, F64, U8 = torch.float16, torch.float32, torch.float64, torch.uint8

# torchvision VGG-16 `features`: conv indices per level (a 2 x 2 max-pool sits between levels), and the widths of the five taps
VGG_LEVELS = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
VGG_WIDTHS = (64, 128, 256, 512, 512)
VGG_CONVS = tuple(i for lv in VGG_LEVELS for i in lv)
MIN_SIDE = 32          # four floor-halvings leave a 2 x 2 last tap
ARENA_BYTES = 4 << 30  # bound of a chunk's activations when no chunk_size is given


def conv_shapes() -> dict:
    """{features index: (cout, cin)} of the 13 convolutions."""
    out, cin = {}, 3
    for lv, c in zip(VGG_LEVELS, VGG_WIDTHS):
        for i in lv:
            out[i] = (c, cin)
            cin = c
    return out


def pair_bytes(H: int, W: int) -> int:
    """Arena bytes of one pair's activations: per level the input operand and two ping-pong outputs, f16, two frames."""
    total, h, w, cin = 0, H, W, CIN_PAD
    for c in VGG_WIDTHS:
        total += h * w * (cin + 2 * c)
        h, w, cin = h // 2, w // 2, c
    return 2 * 2 * total


class LpipsEngine(_EngineBase):
    NEEDS_GPU = "LPIPS runs only on an AMD GPU (no CPU fallback): call .to('cuda')"

    def __init__(self, weights, chunk_size: int | None = None):
        super().__init__(weights, group_norms=False)
        if chunk_size is not None and int(chunk_size) < 1:
            raise ValueError(f"chunk_size: pairs per pass, >= 1; got {chunk_size}")
        self.chunk_size = None if chunk_size is None else int(chunk_size)
        sd = {k: v.detach().to(self.device) for k, v in weights.state_dict().items()}
        W = {}
        for i in VGG_CONVS:
            w = sd[f"features.{i}.weight"].float()
            W[f"c{i}.w"] = pack_conv3x3(w, cin_pad=CIN_PAD if i == 0 else None)
            W[f"c{i}.b"] = sd[f"features.{i}.bias"].float().contiguous()
        for k, c in enumerate(VGG_WIDTHS):
            W[f"lin{k}"] = sd[f"lin{k}.model.1.weight"].float().reshape(c).contiguous()
        self.W = W

    def _chunk(self, n: int, H: int, W: int) -> int:
        return min(n, self.chunk_size or max(1, ARENA_BYTES // pair_bytes(H, W)))

    @torch.no_grad()
    def layers(self, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        """a, b: both uint8 (n,H,W,3) or both fp32 (n,3,H,W), images dense inside -> fp64 (n,5): per pair and tap the mean over
        the tap's pixels of the layer distance.  LPIPS is the sum over the 5 columns."""
        require_cuda(a, b)
        n = a.shape[0]
        H, W = (a.shape[1], a.shape[2]) if a.dtype == U8 else (a.shape[2], a.shape[3])
        if H < MIN_SIDE or W < MIN_SIDE:
            raise ValueError(f"LPIPS (VGG-16) needs H, W >= {MIN_SIDE} (four 2 x 2 pools), got {H} x {W}")
        cs = self._chunk(n, H, W)
        out = torch.empty((n, 5), dtype=F64, device=self.device)
        for i in range(0, n, cs):
            out[i:i + cs] = self._chunk_layers(a[i:i + cs], b[i:i + cs], cs, H, W)
        return out

    def _chunk_layers(self, a, b, cs, H, W):
        """One pass over m <= cs pairs; the buffers are views of the arena's cs-pair tensors."""
        Wt, m = self.W, a.shape[0]
        sums = self._buf("sums", (5, cs), F64)
        h, w, cin = H, W, CIN_PAD
        x = self._buf("in0", (2 * cs, h, w, cin), F16)[:2 * m]
        ops.lpips_prepare(a, x[:m])
        ops.lpips_prepare(b, x[m:])
        for k, (lv, c) in enumerate(zip(VGG_LEVELS, VGG_WIDTHS)):
            nxt = None
            if k + 1 < len(VGG_LEVELS):
                nxt = self._buf(f"in{k + 1}", (2 * cs, h // 2, w // 2, c), F16)[:2 * m]
            for j, i in enumerate(lv):
                y = self._buf(f"out{k}{'ab'[j % 2]}", (2 * cs, h, w, c), F16)[:2 * m]
                ops.conv3x3(x, Wt[f"c{i}.w"], bias=Wt[f"c{i}.b"], out_f16=y.view(2 * m, h * w, c))
                ops.lpips_relu_pool(y, y, nxt if i == lv[-1] else None)
                x = y
            f = x.view(2 * m, h * w, c)
            ws = self._buf("layer_ws", (ops.lpips_layer_workspace_numel(cs, H * W),), U8)
            ops.lpips_layer(f[:m], f[m:], Wt[f"lin{k}"], sums[k, :m], ws)
            sums[k, :m] /= float(h * w)
            x, h, w = nxt, h // 2, w // 2
        return sums[:, :m].t()
