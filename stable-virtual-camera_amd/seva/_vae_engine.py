"""HIP execution of the SD-2.1 VAE: decoder (reference seva/modules/autoencoder.py:37-48 -> diffusers
AutoencoderKL.decode) and encoder (autoencoder.py:21-35 -> AutoencoderKL.encode(x).latent_dist.mean).  Same kernels and layout rules as the UNet engine: channels-last
fp32 stream, fp16 GEMM operands, 3x3 convs as implicit GEMM with the nearest-2x upsample fused
into the gather.  The single-head d=512 mid-block attention runs as GEMM(QK^T) -> row softmax ->
GEMM(P V^T) with V produced already transposed by swapping the GEMM operand roles; the value
bias is added after P*V (rows of P sum to 1, exact).

The decoder's three upsample convs can run as four 2x2 phase convs on the source image (`AutoEncoder.set_upsample("phases")`, or
SEVA_VAE_UPSAMPLE_PHASES=1 when that was not called): see `VaeDecoderEngine.phase_weights`.

The decoder has an opt-in fp8 precision (`AutoEncoder.set_precision("fp8")`, or SEVA_VAE_PRECISION=fp8 when that was not
called): see `fp8_decoder_convs`.  The encoder has one of its own (`AutoEncoder.set_precision(..., encode="fp8")`, or
SEVA_VAE_ENCODE_PRECISION=fp8 when no `encode=` was given): see `fp8_encoder_convs`.
"""

from __future__ import annotations

import os

import torch

from . import audit, ops
from ._engine import CIN_PAD, Act, _EngineBase, combine_up_phases, env_flag, pack_conv3x3
from ._native import require_cuda
from .ops import audit_mark  # (bound here: the tests' seam swaps this module's `ops`)

F16, F32 = torch.float16, torch.float32
U8 = torch.uint8  # e4m3 bytes (ops.py)
VAE_PRECISIONS = ("f16", "fp8")
VAE_UPSAMPLES = ("taps", "phases")


def check_vae_precision(precision: str) -> str:
    if precision not in VAE_PRECISIONS:
        raise ValueError(f"unknown VAE precision {precision!r} (f16 | fp8)")
    return precision


def vae_precision_from_env() -> str:
    """SEVA_VAE_PRECISION=f16|fp8 (unset: f16); used only where `AutoEncoder.set_precision` was not called."""
    return check_vae_precision(os.environ.get("SEVA_VAE_PRECISION") or "f16")


def vae_encode_precision_from_env() -> str:
    """SEVA_VAE_ENCODE_PRECISION=f16|fp8 (unset: f16); used only where `AutoEncoder.set_precision` was not given `encode=`."""
    return check_vae_precision(os.environ.get("SEVA_VAE_ENCODE_PRECISION") or "f16")


def check_vae_upsample(upsample: str) -> str:
    if upsample not in VAE_UPSAMPLES:
        raise ValueError(f"unknown VAE upsample mode {upsample!r} (taps | phases)")
    return upsample


def vae_upsample_from_env() -> str:
    """SEVA_VAE_UPSAMPLE_PHASES=1: "phases" (unset or anything else: "taps"); used only where `AutoEncoder.set_upsample` was not called."""
    return "phases" if env_flag("SEVA_VAE_UPSAMPLE_PHASES", "is1") else "taps"


def up_phases128_applies(ih: int, iw: int) -> bool:
    """Whether `ops.conv3x3_up_phases128` takes a source image of ih x iw pixels (the window kernel's rule, from one image's dimensions):
    linear tiles where the window of every 128-pixel tile of the image -- its pixels in the padded index space, row pitch iw + 1, plus
    a halo of one padded row and one pixel on either side -- fits 288 pixels, else 2-D tiles of 16 x 8 source pixels."""
    if ih < 2 or iw < 2:
        return False
    wp, hw = iw + 1, ih * iw

    def padded(m):
        return (m // iw + 1) * wp + m % iw + 1

    if all(padded(min(m0 + 128, hw) - 1) - padded(m0) + 2 * wp + 3 <= 288 for m0 in range(0, hw, 128)):
        return True
    return iw % 16 == 0 and ih % 8 == 0


def fp8_downsample_from_env() -> bool:
    """SEVA_VAE_FP8_DOWNSAMPLE=1: the fp8 encode also runs the three downsample convs in e4m3 (off by default, see fp8_encoder_convs)."""
    return env_flag("SEVA_VAE_FP8_DOWNSAMPLE", "is1")


def fp8_upsample_from_env() -> bool:
    """SEVA_VAE_FP8_UPSAMPLE=1: the fp8 decode also runs the three upsample convs in e4m3 (off by default, see fp8_decoder_convs)."""
    return env_flag("SEVA_VAE_FP8_UPSAMPLE", "is1")


def fp8_decoder_convs(block_out, upsample: bool = False) -> list[str]:
    """Decoder convs that the fp8 decode runs on e4m3 operands (e4m3 weights with a per-output-channel power-of-two E8M0
    scale, e4m3 activations, fp32 accumulation): every 3x3 conv inside a resnet with cin % 128 == 0 and cout % 128 == 0, i.e.
    both convs of the mid-block resnets and conv1 / conv2 of the up-block resnets.  These stay f16:
      * post_quant_conv (1x1, 4 channels) and decoder.conv_in (4 input channels), decoder.conv_out (3 output channels);
      * the mid-block attention GEMMs;
      * conv2 of the channel-changing resnets (512 -> 256, 256 -> 128): the 1x1 shortcut folded into it (seva_gemm_desc.a2)
        is f16-only;
      * the three upsample convs, unless `upsample` (SEVA_VAE_FP8_UPSAMPLE=1).  Their A operand is the residual stream itself,
        not a normalised resnet branch: in e4m3 its rounding goes straight into every later layer, and the decode's rel-L2 to
        f16 grows about threefold.  With `upsample`, the last resnet of an up
        block writes `conv + residual` as e4m3 straight into the upsample conv's A operand (the e4m3 twin of `f16_out`);
        without, its e4m3 conv2 writes that f16 operand.
    The GroupNorm + SiLU in front of an e4m3 conv writes e4m3."""
    def ok(ci, co):
        return ci % 128 == 0 and co % 128 == 0

    top = block_out[-1]
    names = []
    for r in range(2):
        if ok(top, top):
            names += [f"decoder.mid_block.resnets.{r}.conv1", f"decoder.mid_block.resnets.{r}.conv2"]
    rev = list(reversed(block_out))
    cin = rev[0]
    for i, cout in enumerate(rev):
        for j in range(3):
            ci = cin if j == 0 else cout
            p = f"decoder.up_blocks.{i}.resnets.{j}"
            if ok(ci, cout):
                names.append(p + ".conv1")
            if ci == cout and ok(cout, cout):
                names.append(p + ".conv2")
        cin = cout
        if upsample and i != len(rev) - 1 and ok(cout, cout):
            names.append(f"decoder.up_blocks.{i}.upsamplers.0.conv")
    return names


def fp8_encoder_convs(block_out, downsample: bool = False) -> list[str]:
    """Encoder convs that the fp8 encode runs on e4m3 operands (the counterpart of `fp8_decoder_convs`): every 3x3 conv inside a
    resnet with cin % 128 == 0 and cout % 128 == 0, i.e. both convs of the down-block resnets and of the mid-block resnets.  These
    stay f16:
      * encoder.conv_in (3 input channels) and the folded encoder.conv_out + quant_conv (4 output channels);
      * the mid-block attention GEMMs;
      * conv2 of the channel-changing resnets (128 -> 256, 256 -> 512): the folded 1x1 shortcut (seva_gemm_desc.a2) is f16-only;
      * the three downsample convs (3x3, stride 2, bottom / right padding), unless `downsample` (SEVA_VAE_FP8_DOWNSAMPLE=1).  Like
        the decoder's upsample convs, their A operand is the residual stream itself.  With `downsample`, the second resnet of a down
        block writes `conv + residual` as e4m3 straight into the downsample conv's A operand; without, its e4m3 conv2 writes that
        f16 operand.
    The GroupNorm + SiLU in front of an e4m3 conv writes e4m3."""
    def ok(ci, co):
        return ci % 128 == 0 and co % 128 == 0

    names = []
    cin = block_out[0]
    for i, cout in enumerate(block_out):
        for j in range(2):
            ci = cin if j == 0 else cout
            p = f"encoder.down_blocks.{i}.resnets.{j}"
            if ok(ci, cout):
                names.append(p + ".conv1")
            if ci == cout and ok(cout, cout):
                names.append(p + ".conv2")
        cin = cout
        if downsample and i != len(block_out) - 1 and ok(cout, cout):
            names.append(f"encoder.down_blocks.{i}.downsamplers.0.conv")
    top = block_out[-1]
    for r in range(2):
        if ok(top, top):
            names += [f"encoder.mid_block.resnets.{r}.conv1", f"encoder.mid_block.resnets.{r}.conv2"]
    return names


def pack_fp8_convs(sd: dict, block_out, upsample: bool = False, names=None) -> dict:
    """{prefix + ".w8": e4m3 bytes [cout, 9 * cin] (K ordered (ky, kx, ci), the UNet's fp8 conv layout), prefix + ".w8e":
    E8M0 scale bytes [cout]} for `names` (default: `fp8_decoder_convs`), quantised from the fp32 weights by `ops.quantize_weight_fp8`."""
    W8 = {}
    for p in fp8_decoder_convs(block_out, upsample) if names is None else names:
        w = sd[p + ".weight"].float()
        W8[p + ".w8"], W8[p + ".w8e"] = ops.quantize_weight_fp8(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1))
    return W8


class _VaeEngineBase(_EngineBase):
    NEEDS_GPU = "AutoEncoder runs only on an AMD GPU (no CPU fallback): call .to('cuda')"
    PREFIXES: tuple = ()       # state_dict key prefixes this half owns
    CONV_IN = CONV_OUT = ""    # first conv (input channels padded to 64) / last conv (handled by the subclass)

    _ops = property(lambda self: ops)  # (this module's `ops`)
    _w8: dict = {}  # e4m3 conv weights of the running decode / encode (fp8 precision), else empty

    def __init__(self, weights):
        super().__init__(weights)
        self.block_out = weights.block_out
        self.out_channels = weights.out_channels
        self.latent = weights.latent_channels
        sd = {k: v.detach().to(self.device) for k, v in weights.state_dict().items() if k.startswith(self.PREFIXES)}
        W = {}

        def conv3(p, cin_pad=None, cout_pad=None):
            w, b = sd[p + ".weight"].float(), sd[p + ".bias"].float()
            if cout_pad and cout_pad > w.shape[0]:
                w = torch.cat([w, w.new_zeros((cout_pad - w.shape[0],) + tuple(w.shape[1:]))], 0)
                b = torch.cat([b, b.new_zeros(cout_pad - b.shape[0])], 0)
            W[p + ".w"], W[p + ".b"] = pack_conv3x3(w, cin_pad), b.contiguous()

        def lin(p, src=None):
            src = src or p
            w = sd[src + ".weight"].float()
            W[p + ".w"] = w.reshape(w.shape[0], -1).to(F16).contiguous()
            W[p + ".b"] = sd[src + ".bias"].float().contiguous()

        def norm(p):
            W[p + ".g"], W[p + ".b"] = sd[p + ".weight"].float().contiguous(), sd[p + ".bias"].float().contiguous()

        for k in list(sd):
            if not k.endswith(".weight"):
                continue
            p = k[: -len(".weight")]
            shp = sd[k].shape
            if len(shp) == 1:
                norm(p)
            elif len(shp) == 2 or shp[-1] == 1:
                if p not in ("post_quant_conv", "quant_conv"):
                    lin(p)
            elif p == self.CONV_IN:
                conv3(p, cin_pad=CIN_PAD)
            elif p == self.CONV_OUT:
                pass  # subclass
            else:
                conv3(p)
        # channel-changing resnets: the 1x1 shortcut conv rides in the K loop of the second 3x3 conv (seva_gemm_desc.a2): one
        # accumulation, and the shortcut result (fp32, up to 576 x 576 x 128 per frame) is neither written nor read back
        self.fold_shortcut = env_flag("SEVA_VAE_FOLD_SHORTCUT", "not0", True)
        for k in list(W):
            if k.endswith(".conv_shortcut.w") and W[k].shape[1] % 64 == 0:
                p = k[: -len(".conv_shortcut.w")]
                W[p + ".conv2.wf"] = torch.cat([W[p + ".conv2.w"], W[k]], 1).contiguous()
                W[p + ".conv2.bf"] = (W[p + ".conv2.b"] + W[p + ".conv_shortcut.b"]).contiguous()
        self.W = W
        self._pack_ends(sd, conv3)

    def _resnet(self, p, x: Act, cout, f16_out=None, f8_out=None):
        """diffusers ResnetBlock2D (no time embedding): GN-SiLU-conv-GN-SiLU-conv + shortcut; returns the `Act`, or with f16_out /
        f8_out that buffer (a resampling conv's operand, no stream tensor).
        f16_out: the block's only consumer is a resampling conv (A operand = f16): the second conv's epilogue rounds
        `conv + shortcut` straight into that buffer -- the same rounding the separate cast pass made -- and the fp32 tensor
        (4 B written, 4 B read back per element at up to 576 x 576 x 256) is never formed.  The shortcut conv's f16 input comes
        out of the first GroupNorm's pass over x (`raw_f16`) instead of a cast pass of its own.
        fp8 decode / encode: a conv with e4m3 weights in `self._w8` reads the e4m3 output of its GroupNorm; f8_out is f16_out's
        e4m3 twin (the upsample / downsample conv's A operand, written by the e4m3 conv2's epilogue, saturating)."""
        audit_mark(p)
        W, W8 = self.W, self._w8
        n, h, w, hw, cin = x.n, x.h, x.w, x.hw, x.c
        f8_1, f8_2 = p + ".conv1.w8" in W8, p + ".conv2.w8" in W8
        assert f8_out is None or f8_2
        a16 = None if f8_1 else self._buf("gn16", (n, hw, cin), F16)
        a8 = self._buf("gn8", (n, hw, cin), U8) if f8_1 else None
        xs16 = self._buf("v_sk16", (n * hw, cin), F16) if cin != cout else None
        self._groupnorm(x, None, W[p + ".norm1.g"], W[p + ".norm1.b"], a16, eps=1e-6, silu=True,
                        raw_f16=None if xs16 is None else xs16.view(n, hw, cin), out_f8=a8)
        mid = self._out32("v_mid", n, h, w, cout)
        if f8_1:
            ops.conv3x3(a8.view(n, h, w, cin), W8[p + ".conv1.w8"], w_exp=W8[p + ".conv1.w8e"], bias=W[p + ".conv1.b"], **mid.dst)
        else:
            ops.conv3x3(a16.view(n, h, w, cin), W[p + ".conv1.w"], bias=W[p + ".conv1.b"], **mid.dst)
        b16 = None if f8_2 else self._buf("gn16", (n, hw, cout), F16)
        b8 = self._buf("gn8", (n, hw, cout), U8) if f8_2 else None
        self._groupnorm(mid, None, W[p + ".norm2.g"], W[p + ".norm2.b"], b16, eps=1e-6, silu=True, out_f8=b8)
        # conv2 + shortcut, in e4m3 or f16, into the one tensor its consumer reads
        xb, w2, e2, b2, res, a2 = b16, W[p + ".conv2.w"], None, W[p + ".conv2.b"], x.t, None
        if f8_2:  # (never a channel-changing resnet: its folded shortcut is f16-only)
            assert cin == cout
            xb, w2, e2 = b8, W8[p + ".conv2.w8"], W8[p + ".conv2.w8e"]
        elif cin != cout:
            if self.fold_shortcut and (p + ".conv2.wf") in W:
                w2, b2, res, a2 = W[p + ".conv2.wf"], W[p + ".conv2.bf"], None, xs16
            else:
                res = self._buf("v_sk32", (n * hw, cout), F32)
                ops.gemm(xs16, W[p + ".conv_shortcut.w"], bias=W[p + ".conv_shortcut.b"], out_f32=res)
        if f8_out is not None:
            out, dst = f8_out, {"out_f8": f8_out.view(n, hw, cout)}
        elif f16_out is not None:
            out, dst = f16_out, {"out_f16": f16_out.view(n, hw, cout)}
        else:
            out = self._out32("out:" + p, n, h, w, cout)
            dst = out.dst
        ops.conv3x3(xb.view(n, h, w, cout), w2, w_exp=e2, bias=b2, residual=res, a2=a2, **dst)
        return out

    def _attention(self, p, x: Act) -> Act:
        """Single-head self-attention over h*w tokens of dim c (diffusers Attention in the VAE mid block)."""
        audit_mark(p)
        W = self.W
        n, h, w, hw, c = x.n, x.h, x.w, x.hw, x.c
        if hw % 4:
            raise ValueError(f"VAE attention needs h*w % 4 == 0 (got {h}x{w}); latents are multiples of 8 per side")
        hw_pad = 64 * ((hw + 63) // 64)
        g16 = self._buf("gn16", (n, hw, c), F16)
        self._groupnorm(x, None, W[p + ".group_norm.g"], W[p + ".group_norm.b"], g16, eps=1e-6, silu=False)
        q = self._buf("v_q", (n * hw, c), F16)
        k = self._buf("v_k", (n * hw, c), F16)
        ops.gemm(g16.view(n * hw, c), W[p + ".to_q.w"], bias=W[p + ".to_q.b"], out_f16=q)
        ops.gemm(g16.view(n * hw, c), W[p + ".to_k.w"], bias=W[p + ".to_k.b"], out_f16=k)
        att = self._buf("v_att", (n * hw, c), F16)
        vT = self._buf("v_vT", (c, hw_pad), F16, zero=True)       # V^T, zero beyond hw
        sc = self._buf("v_sc", (hw, hw_pad), F32)
        pr = self._buf("v_pr", (hw, hw_pad), F16)
        for i in range(n):
            gi = g16.view(n, hw, c)[i]
            ops.gemm(W[p + ".to_v.w"], gi, out_f16=vT)             # [c, hw] = W_v @ x_i^T (bias folded below)
            ops.gemm(q[i * hw:(i + 1) * hw], k[i * hw:(i + 1) * hw], out_f32=sc)
            ops.softmax_rows(sc, pr, hw, 1.0 / (c**0.5))
            ops.gemm(pr, vT, bias=W[p + ".to_v.b"], out_f16=att[i * hw:(i + 1) * hw])
        out = self._out32("out:" + p, n, h, w, c)
        ops.gemm(att, W[p + ".to_out.0.w"], bias=W[p + ".to_out.0.b"], residual=x.t2, **out.dst2)
        return out


class VaeDecoderEngine(_VaeEngineBase):
    PREFIXES = ("decoder.", "post_quant_conv.")
    CONV_IN, CONV_OUT = "decoder.conv_in", "decoder.conv_out"

    def __init__(self, weights, precision: str = "f16", upsample: str | None = None):
        super().__init__(weights)
        self.precision = check_vae_precision(precision)  # decode precision; may be changed between decodes (AutoEncoder.set_precision)
        # "taps" | "phases"; may be changed between decodes (AutoEncoder.set_upsample).  None: the environment, read here
        self.upsample = vae_upsample_from_env() if upsample is None else check_vae_upsample(upsample)
        self._src = weights
        self.fp8_upsample = fp8_upsample_from_env()
        self.W8 = None  # e4m3 conv weights, packed the first time an fp8 decode runs
        self.W4 = None  # phase weights of the upsample convs, packed the first time a "phases" decode runs

    def phase_weights(self) -> dict:
        """{prefix + ".w4": f16 [4, cout, 4 * cin]} (`combine_up_phases`: one rounding of the fp64 sums) for the f16 upsample convs that the
        "phases" decode runs through `ops.conv3x3_up_phases128`: those with cout % 128 == 0 (the kernel's tile width; a per-conv rule, so a
        narrower conv of the same decoder keeps the nine-tap call)."""
        if self.W4 is None:
            sd = self._src.state_dict()
            self.W4 = {}
            for i, cout in enumerate(reversed(self.block_out)):
                p = f"decoder.up_blocks.{i}.upsamplers.0.conv"
                if i != len(self.block_out) - 1 and cout % 128 == 0:
                    self.W4[p + ".w4"] = combine_up_phases(sd[p + ".weight"].detach().to(self.device).float())
        return self.W4

    def fp8_weights(self) -> dict:
        if self.W8 is None:
            sd = self._src.state_dict()
            self.W8 = pack_fp8_convs({k: v.detach().to(self.device) for k, v in sd.items() if k.startswith("decoder.")},
                                     self.block_out, self.fp8_upsample)
        return self.W8

    def _pack_ends(self, sd, conv3):
        conv3("decoder.conv_out", cout_pad=4)
        # post_quant_conv (1x1, 4->4) as a GEMM over the 64-channel padded latent image
        wq = torch.zeros((self.latent, CIN_PAD), dtype=F16, device=self.device)
        wq[:, : self.latent] = sd["post_quant_conv.weight"].reshape(self.latent, self.latent).to(F16)
        self.W["post_quant_conv.w"], self.W["post_quant_conv.b"] = wq, sd["post_quant_conv.bias"].float().contiguous()

    @audit.first_call
    @torch.no_grad()
    def decode(self, z: torch.Tensor, scale_factor: float) -> torch.Tensor:
        require_cuda(z)
        audit_mark("post_quant_conv")
        W = self.W
        z = z.to(F32).contiguous()
        n, cz, h, w = z.shape
        if cz != self.latent:
            raise ValueError(f"expected {self.latent} latent channels, got {cz}")
        self.gn_ws = self._buf("gn_ws", (n * ops.GN_WORKSPACE_SLABS * 32 * 2,), F32)
        self._w8 = W8 = self.fp8_weights() if check_vae_precision(self.precision) == "fp8" else {}
        # the upsample convs as four 2x2 phase convs (4/9 of the FLOPs), where the operator exists: the f16 ones only
        phases = getattr(ops, "conv3x3_up_phases128", None) if check_vae_upsample(self.upsample) == "phases" else None
        W4 = self.phase_weights() if phases is not None else {}
        inv = torch.full((n,), 1.0 / scale_factor, dtype=F32, device=self.device)
        z16 = self._buf("v_z16", (n, h * w, CIN_PAD), F16)
        ops.nchw_to_nhwc_f16(z, None, z16, scale=inv)                      # z / 0.18215, channels-last, padded
        pq = self._buf("v_pq16", (n * h * w, CIN_PAD), F16, zero=True)      # cols >= 4 stay zero
        ops.gemm(z16.view(n * h * w, CIN_PAD), W["post_quant_conv.w"], bias=W["post_quant_conv.b"], out_f16=pq)
        top = self.block_out[-1]
        audit_mark("decoder.conv_in")
        x = self._out32("out:conv_in", n, h, w, top)
        ops.conv3x3(pq.view(n, h, w, CIN_PAD), W["decoder.conv_in.w"], bias=W["decoder.conv_in.b"], **x.dst)
        x = self._resnet("decoder.mid_block.resnets.0", x, top)
        x = self._attention("decoder.mid_block.attentions.0", x)
        x = self._resnet("decoder.mid_block.resnets.1", x, top)
        rev = list(reversed(self.block_out))
        for i, cout in enumerate(rev):
            up = i != len(rev) - 1
            p = f"decoder.up_blocks.{i}.upsamplers.0.conv"
            # e4m3 upsample conv (SEVA_VAE_FP8_UPSAMPLE=1): its A operand is written by the e4m3 epilogue of the last resnet's conv2
            up8 = up and p + ".w8" in W8 and f"decoder.up_blocks.{i}.resnets.2.conv2.w8" in W8
            x16 = self._buf("v_up16", (n, h, w, cout), F16) if up and not up8 else None
            x8 = self._buf("v_up8", (n, h, w, cout), U8) if up8 else None
            for j in range(3):
                x = self._resnet(f"decoder.up_blocks.{i}.resnets.{j}", x, cout,
                                 f16_out=x16 if j == 2 else None, f8_out=x8 if j == 2 else None)
            if up:
                h, w = 2 * h, 2 * w
                audit_mark(p)
                x = self._out32("out:" + p, n, h, w, cout)
                if up8:
                    ops.conv3x3(x8, W8[p + ".w8"], w_exp=W8[p + ".w8e"], upsample=True, bias=W[p + ".b"], **x.dst)
                elif p + ".w4" in W4 and up_phases128_applies(h // 2, w // 2):  # (a per-image rule; else the nine taps)
                    # statistics as for the nine taps, where a block of 64 source pixels of one phase stays inside an image (every latent
                    # whose sides are multiples of 8); else the consuming GroupNorm runs its own pass
                    if (h * w // 4) % ops.STATS_ROWS:
                        x.stats = None
                    phases(x16, W4[p + ".w4"], bias=W[p + ".b"], **x.dst, alg_k=9 * cout)
                else:
                    ops.conv3x3(x16, W[p + ".w"], upsample=True, bias=W[p + ".b"], **x.dst)
        c = rev[-1]
        audit_mark("decoder.conv_norm_out")
        g16 = self._buf("gn16", (n, h * w, c), F16)
        self._groupnorm(x, None, W["decoder.conv_norm_out.g"], W["decoder.conv_norm_out.b"], g16, eps=1e-6, silu=True)
        o4 = self._buf("v_o4", (n, h * w, 4), F32)
        ops.conv3x3(g16.view(n, h, w, c), W["decoder.conv_out.w"], bias=W["decoder.conv_out.b"], out_f32=o4)
        out = torch.empty((n, self.out_channels, h, w), dtype=F32, device=self.device)
        ops.nhwc_to_nchw_f32(o4, out)
        return out


class VaeEncoderEngine(_VaeEngineBase):
    """x (n,3,H,W) in [-1,1] -> mean latent * scale_factor (n,4,H/8,W/8).  `quant_conv` (1x1) is folded into
    `encoder.conv_out` at pack time in fp64 and only the mean half of the moments is produced."""

    PREFIXES = ("encoder.", "quant_conv.")
    CONV_IN, CONV_OUT = "encoder.conv_in", "encoder.conv_out"

    def __init__(self, weights, precision: str = "f16"):
        super().__init__(weights)
        self.precision = check_vae_precision(precision)  # encode precision; may be changed between encodes (AutoEncoder.set_precision)
        self._src = weights
        self.fp8_downsample = fp8_downsample_from_env()
        self.W8 = None  # e4m3 conv weights, packed the first time an fp8 encode runs

    def fp8_weights(self) -> dict:
        if self.W8 is None:
            sd = self._src.state_dict()
            self.W8 = pack_fp8_convs({k: v.detach().to(self.device) for k, v in sd.items() if k.startswith("encoder.")},
                                     self.block_out, names=fp8_encoder_convs(self.block_out, self.fp8_downsample))
        return self.W8

    def _pack_ends(self, sd, conv3):
        L = self.latent
        wo, bo = sd["encoder.conv_out.weight"].double(), sd["encoder.conv_out.bias"].double()
        wq = sd["quant_conv.weight"].double().reshape(2 * L, 2 * L)[:L]  # mean rows only
        w = (wq @ wo.reshape(2 * L, -1)).reshape(L, *wo.shape[1:])
        b = wq @ bo + sd["quant_conv.bias"].double()[:L]
        self.W["enc_out.w"], self.W["enc_out.b"] = pack_conv3x3(w.float()), b.float().contiguous()

    @audit.first_call
    @torch.no_grad()
    def encode(self, x: torch.Tensor, scale_factor: float) -> torch.Tensor:
        require_cuda(x)
        audit_mark("encoder.conv_in")
        W = self.W
        x = x.to(F32).contiguous()
        n, cx, h, w = x.shape
        nd = len(self.block_out) - 1
        if h % (1 << nd) or w % (1 << nd):
            raise ValueError(f"VAE encode needs H and W divisible by {1 << nd} (got {h}x{w})")
        self.gn_ws = self._buf("gn_ws", (n * ops.GN_WORKSPACE_SLABS * 32 * 2,), F32)
        self._w8 = W8 = self.fp8_weights() if check_vae_precision(self.precision) == "fp8" else {}
        one = torch.ones((n,), dtype=F32, device=self.device)
        x16 = self._buf("v_x16", (n, h * w, CIN_PAD), F16)
        ops.nchw_to_nhwc_f16(x, None, x16, scale=one)  # channels-last, 3 -> 64 zero-padded channels
        c0 = self.block_out[0]
        cur = self._out32("out:enc_in", n, h, w, c0)
        ops.conv3x3(x16.view(n, h, w, CIN_PAD), W["encoder.conv_in.w"], bias=W["encoder.conv_in.b"], **cur.dst)
        for i, cout in enumerate(self.block_out):
            p = f"encoder.down_blocks.{i}.downsamplers.0.conv"
            # e4m3 downsample conv (SEVA_VAE_FP8_DOWNSAMPLE=1): its A operand is written by the e4m3 epilogue of the second resnet's conv2
            dn8 = i != nd and p + ".w8" in W8 and f"encoder.down_blocks.{i}.resnets.1.conv2.w8" in W8
            d16 = self._buf("v_dn16", (n, h, w, cout), F16) if i != nd and not dn8 else None
            d8 = self._buf("v_dn8", (n, h, w, cout), U8) if dn8 else None
            for j in range(2):
                cur = self._resnet(f"encoder.down_blocks.{i}.resnets.{j}", cur, cout,
                                   f16_out=d16 if j == 1 else None, f8_out=d8 if j == 1 else None)
            if i != nd:
                h, w = h // 2, w // 2
                audit_mark(p)
                cur = self._out32("out:" + p, n, h, w, cout)
                if dn8:
                    ops.conv3x3(d8, W8[p + ".w8"], w_exp=W8[p + ".w8e"], stride=2, pad_br_only=True, bias=W[p + ".b"], **cur.dst)
                else:
                    ops.conv3x3(d16, W[p + ".w"], stride=2, pad_br_only=True, bias=W[p + ".b"], **cur.dst)
        top = self.block_out[-1]
        cur = self._resnet("encoder.mid_block.resnets.0", cur, top)
        cur = self._attention("encoder.mid_block.attentions.0", cur)
        cur = self._resnet("encoder.mid_block.resnets.1", cur, top)
        audit_mark("encoder.conv_norm_out")
        g16 = self._buf("gn16", (n, h * w, top), F16)
        self._groupnorm(cur, None, W["encoder.conv_norm_out.g"], W["encoder.conv_norm_out.b"], g16, eps=1e-6, silu=True)
        o4 = self._buf("v_m4", (n, h * w, self.latent), F32)
        ops.conv3x3(g16.view(n, h, w, top), W["enc_out.w"], bias=W["enc_out.b"], out_f32=o4)
        out = torch.empty((n, self.latent, h, w), dtype=F32, device=self.device)
        ops.nhwc_to_nchw_f32(o4, out)
        ops.scale_rows(out, torch.full((n,), float(scale_factor), dtype=F32, device=self.device), out)
        return out
