"""HIP execution engine behind `seva.model.Seva.forward` (reference seva/model.py:176-216).

Packs the module's parameters once into kernel-friendly fp16/fp32 device buffers and then runs
the UNet as a fixed sequence of C-ABI kernel launches (`seva.ops`) on PyTorch's current stream.
All intermediate buffers come from a per-shape arena that is filled on the first call, so a
second call performs no allocation and can be captured into a hipGraph (`ops.Graph`).

Data layout in HBM: channels-last activations; fp32 residual stream
[N][h*w][C]; every GEMM/conv A-operand is an fp16 tensor written by the producing norm /
activation / attention kernel; weights fp16 [N_out][K] with K = (ky,kx,ci) for 3x3 convs.

Exact algebraic rewrites (each checked against the oracle in tests/):
  * cross-attention with ONE context token (the only case `do_sample` produces, reference
    eval.py:1248 / transformer.py:222-226): softmax over one key is 1, so
    attn2(x, ctx) == to_out(to_v(ctx)) for every query; W_out @ W_v is folded at pack time and all
    32 such vectors are produced by one GEMM per forward.  Longer contexts take the general
    path (`_cross_attention_general`).
  * the skip concat (model.py:206-207) is never materialised for GroupNorm (two-source reads).
  * `(b t) s c <-> (b s) t c` transposes of the time-mix block (transformer.py:149,154) vanish:
    token-wise ops run in place and the temporal attention reads through strides.
"""

from __future__ import annotations

import math
import os

import torch

from . import _native, audit, ops
from ._arch import Layout
from ._native import SevaNativeError, require_cuda
from .ops import audit_mark  # (bound here: the tests' seam swaps this module's `ops` for kernel emulations)
from .ops import SPLITK_ERROR_SLOT, SPLITK_MAX_PIXELS, splitk_tiles, splitk_workspace_numel  # (likewise: contract arithmetic, no kernel)

F16, F32, U8 = torch.float16, torch.float32, torch.uint8
# softmax scale of head dim 64 (reference transformer.py:66-72) times log2(e): exp(x) == exp2(x * log2 e)
QK_SCALE_LOG2E = 0.125 * 1.4426950408889634
CIN_PAD = 64  # conv A-operand channel granularity (one K-tile per tap)


# --------------------------------------------------------------------------- weight packing
def _pad128(k: int) -> int:
    return 128 * ((k + 127) // 128)


def pack_conv3x3(w: torch.Tensor, cin_pad: int | None = None) -> torch.Tensor:
    """[cout, cin, 3, 3] -> f16 [cout, 9*cin_pad], K ordered (ky, kx, ci); extra channels zero."""
    cout, cin = w.shape[:2]
    cin_pad = cin_pad or cin
    out = torch.zeros((cout, 3, 3, cin_pad), dtype=F16, device=w.device)
    out[..., :cin] = w.permute(0, 2, 3, 1).to(F16)
    return out.reshape(cout, 9 * cin_pad).contiguous()


def combine_up_phases(w: torch.Tensor, dtype: torch.dtype = F16) -> torch.Tensor:
    """[cout, cin, 3, 3] fp32 -> f16 [4, cout, 4*cin]: the weights of `ops.conv3x3_up_phases`.  After a nearest-2x upsample, output
    row 2i + py reads source rows {i-1, i, i} (py = 0) or {i, i, i+1} (py = 1), columns alike, so output phase (py, px) is a 2x2 conv
    on the source image whose tap (a, b) sits at source offset (a + py - 1, b + px - 1) and carries the sum of the 3x3 weights that
    meet there:

        py = 0:  a = 0 <- W[0]         a = 1 <- W[1] + W[2]
        py = 1:  a = 0 <- W[0] + W[1]  a = 1 <- W[2]

    Summed in fp64 from the fp32 weights and rounded to f16 ONCE (summing f16-rounded weights would round twice).  Phase
    2 py + px, K ordered (a, b, ci).  (`dtype`: the tests look at the sums before the rounding.)"""
    fold = ((0,), (1, 2)), ((0, 1), (2,))  # fold[p][a]: the 3x3 rows (columns) that meet on tap a of phase p
    w64 = w.double()
    cout, cin = w.shape[:2]
    out = torch.empty((4, cout, 2, 2, cin), dtype=dtype, device=w.device)
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    out[2 * py + px, :, a, b] = w64[:, :, list(fold[py][a])][:, :, :, list(fold[px][b])].sum((2, 3)).to(dtype)
    return out.reshape(4, cout, 4 * cin).contiguous()


def interleave_geglu(w: torch.Tensor, b: torch.Tensor):
    """Reorder GEGLU projection rows (value rows 0..Nh-1, gate rows Nh..2Nh-1, reference
    transformer.py:13-14) into groups of 64 = [32 value | 32 gate] (include/seva_hip.h)."""
    nh = w.shape[0] // 2
    g = nh // 32
    wi = torch.stack([w[:nh].reshape(g, 32, -1), w[nh:].reshape(g, 32, -1)], 1).reshape(2 * nh, -1)
    bi = torch.stack([b[:nh].reshape(g, 32), b[nh:].reshape(g, 32)], 1).reshape(2 * nh)
    return wi.contiguous(), bi.contiguous()


# Split-precision operand classes (SEVA_SPLIT_PRECISION / Seva.set_precision(split=...)): the operand travels as [hi | lo] f16 pairs
# against weights duplicated [W | W] -- K doubles, no consumer kernel changes
SPLIT_TOKENS = ("stem", "head", "skip", "skip_deep", "conv", "resample", "proj_in", "proj_out", "qkv", "ff")
SPLIT_ALL = frozenset(t for t in SPLIT_TOKENS if t != "skip_deep")  # "all" ("skip" covers "skip_deep")
SPLIT_DEFAULT = "stem,head,skip_deep"


def parse_split(spec, strict: bool = False) -> set:
    """Token set of a split-precision request: a comma list (or a sequence) of SPLIT_TOKENS, "all" = every class, "none" / "" = every
    operand plain fp16.  strict (the `split=` keyword): an unknown token is a ValueError; the environment variable stays lenient."""
    toks = [t.strip() for t in (spec.split(",") if isinstance(spec, str) else list(spec))]
    toks = [t for t in toks if t]
    if strict:
        bad = [t for t in toks if t not in SPLIT_TOKENS + ("all", "none")]
        if bad:
            raise ValueError(f"unknown split-precision token(s) {bad} (any of {', '.join(SPLIT_TOKENS)}, or all / none)")
    out = set(toks)
    if "all" in out:
        out = (out - {"all"}) | SPLIT_ALL
    return out


def dup_k(w: torch.Tensor) -> torch.Tensor:
    """[N, K] -> [N, 2K] = [W | W]: the weights a split-precision [hi | lo] operand meets (a conv weight [cout, cin, 3, 3]: along cin)."""
    return torch.cat([w, w], 1).contiguous()


class _Arena:
    """Shape-keyed buffer cache: the second forward of a shape allocates nothing."""

    def __init__(self, device):
        self.device = device
        self.bufs: dict = {}
        audit.register_arena(self)  # (weakly: the audit names the buffer an output lies in)

    def get(self, name: str, shape, dtype, zero: bool = False) -> torch.Tensor:
        """zero: zeroed once, when the buffer is made (pad columns that nothing writes again, flag areas)"""
        key = (name, tuple(int(s) for s in shape), dtype)
        t = self.bufs.get(key)
        if t is None:
            t = self.bufs[key] = (torch.zeros if zero else torch.empty)(key[1], dtype=dtype, device=self.device)
        return t

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.bufs.values())


def env_flag(name: str, rule: str, default: bool = False) -> bool:
    """Boolean switch `name`; unset: `default`.  rule "not0": on at anything but "0"; rule "is1": on at exactly "1"."""
    v = os.environ.get(name)
    return default if v is None else (v != "0" if rule == "not0" else v == "1")


def env_int(name: str, default: int) -> int:
    return int(os.environ.get(name, default))


class Act:
    """A residual-stream tensor on its way from block to block: `t`, fp32 channels-last [n, h*w, c], the image size, and `stats`,
    the GroupNorm statistics that its producer's epilogue emitted (seva_gemm_desc.ch_stats), or None where it emitted none."""

    __slots__ = ("t", "n", "h", "w", "stats")

    def __init__(self, t, n, h, w, stats=None):
        self.t, self.n, self.h, self.w, self.stats = t, n, h, w, stats

    hw = property(lambda self: self.h * self.w)
    c = property(lambda self: self.t.shape[2])
    rows = property(lambda self: self.n * self.h * self.w)
    t2 = property(lambda self: self.t.view(self.rows, self.c))  # [rows, c]: what a GEMM reads or writes
    # the output keywords of the call that produces it: a conv (3-D), a GEMM (2-D)
    dst = property(lambda self: {"out_f32": self.t, "ch_stats": self.stats})
    dst2 = property(lambda self: {"out_f32": self.t2, "ch_stats": self.stats})


class _EngineBase:
    """What the UNet, VAE and CLIP engines share: the device of the module they pack, the arena, and (engines with GroupNorms) the
    hand-off of GroupNorm statistics from the producing kernel's epilogue."""

    NEEDS_GPU = ""  # the error of a module that is not on a cuda device
    _ops = property(lambda self: ops)  # what `_groupnorm` launches through: an engine in another module binds its own `ops` (the tests' seam)

    @staticmethod
    def _resolve_device(module):
        """The module's cuda device (the library is loaded on the way), None if it is not on one.  (One argument: the tests' seam.)"""
        params = list(module.parameters())
        if not params or params[0].device.type != "cuda":
            return None
        _native.load()
        return params[0].device

    def __init__(self, module, group_norms: bool = True):
        self.device = self._resolve_device(module)
        if self.device is None:
            raise SevaNativeError(self.NEEDS_GPU)
        self.arena = _Arena(self.device)
        if group_norms:
            # GroupNorm statistics from the producers' epilogues: 0 off (separate statistics pass everywhere, A/B runs),
            # 1 where it pays (default), 2 wherever hw % 64 == 0, even on launches that would otherwise run 64-row tiles (tests)
            self.gn_fused_stats = env_int("SEVA_GN_FUSED_STATS", 1)

    def _buf(self, name, shape, dtype, zero=False):
        return self.arena.get(name, shape, dtype, zero)

    # GroupNorm statistics emitted by the producing kernel's epilogue (seva_gemm_desc.ch_stats): a tensor that a GroupNorm will
    # read gets a [rows / 64][2][c] side buffer filled by the conv / GEMM that writes it, and that GroupNorm then skips its
    # statistics pass over the fp32 tensor.  Only where a 64-row block cannot straddle two samples (hw % 64 == 0: results stay
    # bitwise independent of the batch composition) and where the launch keeps 128-row tiles anyway.
    def _stats_buf(self, name, rows, hw, c):
        if not self.gn_fused_stats or hw % ops.STATS_ROWS or c < 128 or c % 4:
            return None
        # small images keep the statistics pass: their launches run 64-row tiles, which have no statistics variant.  The rule
        # looks at ONE sample (never at the batch size): a sample's result must not depend on what it is batched with
        if self.gn_fused_stats < 2 and (hw // 128) * ((c + 159) // 160) < 16:
            return None
        return self._buf("st:" + name, ops.channel_stats_shape(rows, c), F32)

    def _out32(self, name, n, h, w, c) -> Act:
        """The arena's stream tensor `name`, with the statistics buffer its producer is to fill (`_stats_buf`'s rule)."""
        t = self._buf(name, (n, h * w, c), F32)
        return Act(t, n, h, w, self._stats_buf(name, n * h * w, h * w, c))

    def _groupnorm(self, x: Act, x2: Act | None, gamma, beta, out_f16, **kw):
        """`ops.groupnorm` over x (|| x2) with the producers' statistics: both sources' buffers, or none unless every source has one."""
        s1, s2 = x.stats, None if x2 is None else x2.stats
        if s1 is None or (x2 is not None and s2 is None):
            s1 = s2 = None
        self._ops.groupnorm(x.t, None if x2 is None else x2.t, gamma, beta, out_f16, self.gn_ws, stats1=s1, stats2=s2, **kw)


class SevaEngine(_EngineBase):
    NEEDS_GPU = "Seva.forward runs only on an AMD GPU: move the module to a cuda device first (there is no CPU fallback)."
    split: frozenset = frozenset()  # split-precision operand classes; set per instance in __init__ (an engine built without it: none)
    _resolve_device = staticmethod(_EngineBase._resolve_device)  # (an entry of its own: tests save and restore `__dict__["_resolve_device"]`)

    def __init__(self, model, precision: str | None = None, attention: str | None = None, ff: str | None = None, split=None):
        """precision "f16" (default; the parity mode, fp16 operands / fp32 accumulation) or "fp8" (BASELINE config 5:
        e4m3 weights AND activations on the block-scaled fp8 MFMA for the QKV / GEGLU / FF2 projections and the ResBlock 3x3
        convs whose reduction length is a multiple of 128 -- the C = 640 / 1280 levels; the C = 320 level (opt-in through
        zero-padding, SEVA_FP8_PAD=1: no gain, see below), attention, the small projections and the resampling convs stay f16).
        split (f16 only): the split-precision operand classes (`parse_split`); None leaves the choice to SEVA_SPLIT_PRECISION."""
        super().__init__(model)
        self.precision = precision or os.environ.get("SEVA_PRECISION", "f16")
        if self.precision not in ("f16", "fp8"):
            raise ValueError(f"unknown precision {self.precision!r} (f16 | fp8)")
        self.fp8 = self.precision == "fp8"
        # fp8 mode's attention sub-option: "fp8" runs the long self-attention launches (lq >= ops.PV8_MIN_LQ, the ones
        # seva_attention_f16 gives attn16_kernel) with P and V in e4m3 (seva_attention_pv8).  Not given: SEVA_FP8_ATTENTION=0|1.
        self.attention = self._fp8_option("attention", attention, "SEVA_FP8_ATTENTION")
        self.pv8 = self.attention == "fp8"
        # fp8 mode only: also take reductions that need zero-padding to a multiple of 128 (C = 320 -> 384, 960 -> 1024).  Off by
        # default -- measured (profiles/r02_bench_T21_fp8_pad320.json): the C = 320 level then leaves the fused f16 feed-forward
        # for the two-kernel fp8 path, the step stays at 86.1 ms and the error doubles (rel-L2 2.9e-2 -> 5.2e-2).
        self.fp8_pad = env_flag("SEVA_FP8_PAD", "is1")
        self.ff_fused = env_flag("SEVA_FF_FUSED", "not0", True)  # 0: two-kernel GEGLU + FF2 everywhere (A/B runs)
        # fp8 mode's feed-forward sub-option: "fp8" runs the feed-forwards that take the fused f16 kernel in fp8 mode (reduction
        # not a multiple of 128: the C = 320 level, the tiny net's C = 64) on its e4m3 sibling (seva_ff_fused_fp8); with
        # SEVA_FP8_PAD=1 it takes precedence over the padded two-kernel chain there.  Not given: SEVA_FP8_FF=0|1.
        self.ff = self._fp8_option("ff", ff, "SEVA_FP8_FF")
        self.ff8 = self.ff == "fp8"
        self.conv_splitk = env_flag("SEVA_CONV_SPLITK", "not0", True)  # 0: 64-row tiles at the 9x9 level (A/B runs)
        self.attn_split = env_flag("SEVA_ATTN_SPLIT_KV", "not0", True)  # 0: joint attention never K/V-split (A/B runs)
        self.attn_split_max = max(2, min(4, env_int("SEVA_ATTN_SPLIT", 2)))  # workspace slots (knob attn_split: 2..4)
        # 1: the ResBlock's 1x1 skip conv as extra K-tiles of its second 3x3 conv (one accumulation, no fp32 round trip of the skip
        # result, a launch fewer).  OFF by default -- measured neutral (profiles/r03_ab_fold_skip.log: 96.9 vs 96.5 ms per step over two
        # interleaved rounds, GEMM class -2.0 ms, conv class +1.2 ms).  Not at levels whose convs run split-K (images <= 128 px).
        self.fold_skip = env_flag("SEVA_FOLD_SKIP", "not0") and not self.fp8
        # Split-precision operands (hi + lo f16 pairs against duplicated weights) for the three operand roundings that dominate the
        # network's error budget (tests/test_f16_floor_cpu.py: 1x1 skip convs 4.9e-4, stem 2.4e-4, head 2.3e-4 of 8.1e-4):
        # comma list of "stem", "head", "skip" / "skip_deep"; "none" = every operand plain fp16 (the round-2 numerics).
        # "skip_deep" = the skip convs below the top level only (cout >= 640: 11 of the 14, where M is small and the doubled K and
        # the extra lo half of the raw input cost ~0.3 ms per step; the three 72x72 ones cost ~0.8 ms for 3.6e-4 of the error budget).
        # The further classes finish the scheme ("all": the near-fp32 mode, every GEMM / conv A operand of the UNet but attention's and
        # the time-embedding MLP's): "conv" (both 3x3 convs of every ResBlock), "resample" (the Down / Upsample convs), "proj_in",
        # "proj_out", "qkv", "ff" (GEGLU-in and FF2; the C <= 320 feed-forwards then take the two-kernel path: the fused kernel has no
        # split hidden tensor).  Each is a per-layer decision from per-sample dimensions only (batch invariance holds).
        if split is not None:
            if self.fp8:
                raise ValueError('split precision needs precision "f16" (the fp8 mode has no split operands)')
            self.split = parse_split(split, strict=True)
        else:  # (fp8 mode: the environment variable is ignored)
            self.split = parse_split(os.environ.get("SEVA_SPLIT_PRECISION", SPLIT_DEFAULT)) if not self.fp8 else set()
        self.p = model.params
        self.layout: Layout = model._layout
        self._pack(model)
        # hipGraph replay of the whole network call (SEVA_HIPGRAPH=0 disables): one captured graph
        # per input signature, fed through static input buffers
        self.use_graph = env_flag("SEVA_HIPGRAPH", "not0", True)
        self._graphs: dict = {}
        # shallow calls (`forward(shallow_levels=L)`): the signature of the last full call, and per signature what a full call
        # left behind for each entry point L -- the `Act` entering the first output block a shallow call runs (statistics included)
        self._last_full: tuple | None = None
        self._shallow_entries: dict = {}
        # per depth L = 1, 2, ...: the input blocks after the stem that precede the L-th Downsample of the layout
        self._shallow_m = tuple(i - 1 for i, blk in enumerate(self.layout.input_blocks) if blk[0].kind == "down")
        # frame-sliced execution of the token-wise chains at the largest level (see _slice_rows); 0 frames = off (default:
        # measured end-to-end it does not pay, see _slice_rows)
        self.slice_frames = env_int("SEVA_SLICE_FRAMES", 0)
        self.slice_min_bytes = int(float(os.environ.get("SEVA_SLICE_MIN_MB", "96")) * (1 << 20))
        self.slice_attn = env_flag("SEVA_SLICE_ATTN", "is1")  # also slice LN -> QKV -> attention -> out-proj

    def _fp8_option(self, name: str, value, switch: str) -> str:
        """The `attention=` / `ff=` sub-option of the fp8 mode, "f16" | "fp8"; None leaves it to the environment `switch` (fp8 mode only)."""
        if value is None:
            value = "fp8" if self.fp8 and env_flag(switch, "is1") else "f16"
        if value not in ("f16", "fp8"):
            raise ValueError(f"unknown {name} {value!r} (f16 | fp8)")
        if value == "fp8" and not self.fp8:
            raise ValueError(f'{name}="fp8" needs precision "fp8" (the f16 parity mode stays pure)')
        return value

    def _ff_fused_fp8(self, c: int) -> bool:
        """Does a feed-forward of width c run on seva_ff_fused_fp8?  Exactly those that reach the fused f16 kernel in fp8 mode
        without SEVA_FP8_PAD (reduction not a multiple of 128), when the ff="fp8" option is on."""
        return self.ff8 and self.ff_fused and c in ops.FF_FUSED_CHANNELS and c % 128 != 0

    def _split_skip(self, cout: int) -> bool:
        """Does the 1x1 skip conv of a ResBlock with `cout` output channels take its raw input in split precision?"""
        return "skip" in self.split or ("skip_deep" in self.split and cout >= 2 * self.p.model_channels)

    # ------------------------------------------------------------------ packing
    def _pack(self, model) -> None:
        sd = {k: v.detach() for k, v in model.state_dict().items()}
        dev = self.device
        W: dict[str, torch.Tensor] = {}

        def f16(k):
            return sd[k].to(device=dev, dtype=F16).contiguous()

        def f32(k):
            return sd[k].to(device=dev, dtype=F32).contiguous()

        mc = self.p.model_channels
        half = mc // 2
        W["freqs"] = torch.exp(
            -math.log(10000) * torch.arange(start=0, end=half, dtype=torch.float32) / half
        ).to(dev)
        for k in ("time_embed.0", "time_embed.2"):
            W[k + ".w"], W[k + ".b"] = f16(k + ".weight"), f32(k + ".bias")

        emb_w, emb_b, ctx_w, ctx_b = [], [], [], []
        self.emb_off: dict[str, int] = {}
        self.ctx_off: dict[str, int] = {}
        emb_total = ctx_total = 0

        def q8(name, w):
            """fp8 mode: e4m3 copy + per-row power-of-two scale bytes of an [N, K] weight; K is zero-padded to a multiple of
            128 (one MFMA K-tile) when that costs at most 25 % (320 -> 384: the producing LayerNorm writes into a zero-padded
            buffer of that width)"""
            if not (self.fp8 and w.shape[0] % 16 == 0 and w.shape[0] > 32):
                return
            k = w.shape[1]
            kp = _pad128(k)
            if kp != k and (not self.fp8_pad or kp * 4 > k * 5):
                return
            if kp != k:
                w = torch.cat([w, w.new_zeros((w.shape[0], kp - k))], 1)
            W[name + "8"], W[name + "8e"] = ops.quantize_weight_fp8(w)

        sp = self.split

        def pack_attn_self(pfx):
            def qkv(conv):
                return torch.cat([conv(pfx + ".to_q.weight"), conv(pfx + ".to_k.weight"), conv(pfx + ".to_v.weight")], 0)

            W[pfx + ".qkv"] = dup_k(qkv(f16)) if "qkv" in sp else qkv(f16)  # ("qkv": the LayerNorm output arrives as [hi | lo])
            if self.fp8:
                q8(pfx + ".qkv", qkv(f32))
            W[pfx + ".out.w"], W[pfx + ".out.b"] = f16(pfx + ".to_out.0.weight"), f32(pfx + ".to_out.0.bias")

        def pack_attn_cross(pfx):
            nonlocal ctx_total
            wv, wo, bo = f32(pfx + ".to_v.weight"), f32(pfx + ".to_out.0.weight"), f32(pfx + ".to_out.0.bias")
            ctx_w.append((wo.double() @ wv.double()).to(F16))  # folded W_out @ W_v  [C, ctx]
            ctx_b.append(bo)
            self.ctx_off[pfx] = ctx_total
            ctx_total += wo.shape[0]
            # general path (context length > 1)
            W[pfx + ".q"] = f16(pfx + ".to_q.weight")
            W[pfx + ".kv"] = torch.cat([f16(pfx + ".to_k.weight"), f16(pfx + ".to_v.weight")], 0).contiguous()
            W[pfx + ".out.w"], W[pfx + ".out.b"] = f16(pfx + ".to_out.0.weight"), bo

        def pack_ff(pfx):
            b1 = f32(pfx + ".net.0.proj.bias")
            wi, bi = interleave_geglu(f16(pfx + ".net.0.proj.weight"), b1)
            W[pfx + ".w1"], W[pfx + ".b1"] = wi, bi
            W[pfx + ".w2"], W[pfx + ".b2"] = f16(pfx + ".net.2.weight"), f32(pfx + ".net.2.bias")
            if "ff" in sp:  # LayerNorm output and GEGLU hidden tensor arrive as [hi | lo]
                W[pfx + ".w1"], W[pfx + ".w2"] = dup_k(W[pfx + ".w1"]), dup_k(W[pfx + ".w2"])
            if not self.fp8:
                return
            wi32 = interleave_geglu(f32(pfx + ".net.0.proj.weight"), b1)[0]
            if self._ff_fused_fp8(wi.shape[1]):  # e4m3 copies for seva_ff_fused_fp8 (W1 zero-padded to KP, W2 column-permuted)
                W[pfx + ".w1f8"], W[pfx + ".w1f8e"], W[pfx + ".w2f8"], W[pfx + ".w2f8e"] = ops.pack_ff_fp8(wi32, f32(pfx + ".net.2.weight"))
            else:  # both or neither: the hidden activations travel as e4m3
                q8(pfx + ".w1", wi32)
                if pfx + ".w18" in W:
                    q8(pfx + ".w2", f32(pfx + ".net.2.weight"))

        def pack_ln(pfx):
            W[pfx + ".g"], W[pfx + ".b"] = f32(pfx + ".weight"), f32(pfx + ".bias")

        for spec in self.layout.all_specs():
            pfx = spec.prefix
            if spec.kind == "conv":
                wc = f32(pfx + ".weight")
                if "stem" in self.split and 2 * spec.cin <= CIN_PAD:  # [w | w]: the input arrives as [hi | lo] channels
                    wc = dup_k(wc)
                W[pfx + ".w"] = pack_conv3x3(wc, CIN_PAD * ((wc.shape[1] + CIN_PAD - 1) // CIN_PAD))
                W[pfx + ".b"] = f32(pfx + ".bias")
            elif spec.kind == "res":
                assert spec.cin % 64 == 0 and spec.cout % 64 == 0, "channel counts must be multiples of 64"
                pack_ln(pfx + ".in_layers.0")
                pack_ln(pfx + ".out_layers.0")
                wc1, wc2 = f32(pfx + ".in_layers.2.weight"), f32(pfx + ".out_layers.3.weight")
                # ("conv": [w | w] per tap, both GroupNorms write [hi | lo] channels)
                W[pfx + ".conv1.w"] = pack_conv3x3(dup_k(wc1) if "conv" in sp else wc1)
                W[pfx + ".conv1.b"] = f32(pfx + ".in_layers.2.bias")
                W[pfx + ".conv2.w"] = pack_conv3x3(dup_k(wc2) if "conv" in sp else wc2)
                W[pfx + ".conv2.b"] = f32(pfx + ".out_layers.3.bias")
                if self.fp8:  # K = 9*cin_pad ordered (ky, kx, ci): a 128-deep K-tile must not straddle taps -> channels padded
                    for tag, wc, ch in (("conv1", wc1, spec.cin), ("conv2", wc2, spec.cout)):
                        cp = _pad128(ch)
                        if cp == ch or (self.fp8_pad and cp * 4 <= ch * 5):
                            q8(f"{pfx}.{tag}.w", pack_conv3x3(wc, cp).float())
                W[pfx + ".dense.w"] = f32(pfx + ".dense_emb_layers.0.weight").reshape(2 * spec.cin, -1).contiguous()
                W[pfx + ".dense.b"] = f32(pfx + ".dense_emb_layers.0.bias")
                emb_w.append(f16(pfx + ".emb_layers.1.weight"))
                emb_b.append(f32(pfx + ".emb_layers.1.bias"))
                self.emb_off[pfx] = emb_total
                emb_total += spec.cout
                if spec.cin != spec.cout:
                    ws = f16(pfx + ".skip_connection.weight").reshape(spec.cout, spec.cin)
                    # split precision: the raw input arrives as [hi | lo] (K = 2 cin), the weights are duplicated
                    W[pfx + ".skip.w"] = dup_k(ws) if self._split_skip(spec.cout) else ws.contiguous()
                    W[pfx + ".skip.b"] = f32(pfx + ".skip_connection.bias")
                    if self.fold_skip:
                        # the skip conv folded into conv2 (seva_gemm_desc.a2): weights [w_conv2 | w_skip] per output row, biases summed
                        W[pfx + ".conv2.wf"] = torch.cat([W[pfx + ".conv2.w"], W[pfx + ".skip.w"]], 1).contiguous()
                        W[pfx + ".conv2.bf"] = (W[pfx + ".conv2.b"] + W[pfx + ".skip.b"]).contiguous()
            elif spec.kind == "mvt":
                pack_ln(pfx + ".norm")
                W[pfx + ".proj_in.w"], W[pfx + ".proj_in.b"] = f16(pfx + ".proj_in.weight"), f32(pfx + ".proj_in.bias")
                W[pfx + ".proj_out.w"], W[pfx + ".proj_out.b"] = f16(pfx + ".proj_out.weight"), f32(pfx + ".proj_out.bias")
                if "proj_in" in sp:
                    W[pfx + ".proj_in.w"] = dup_k(W[pfx + ".proj_in.w"])
                if "proj_out" in sp:
                    W[pfx + ".proj_out.w"] = dup_k(W[pfx + ".proj_out.w"])
                for i in range(spec.depth):
                    b = f"{pfx}.transformer_blocks.{i}"
                    pack_attn_self(b + ".attn1")
                    pack_attn_cross(b + ".attn2")
                    pack_ff(b + ".ff")
                    for n in ("norm1", "norm2", "norm3"):
                        pack_ln(f"{b}.{n}")
                    m = f"{pfx}.time_mix_blocks.{i}"
                    pack_attn_self(m + ".attn1")
                    pack_attn_cross(m + ".attn2")
                    pack_ff(m + ".ff_in")
                    pack_ff(m + ".ff")
                    for n in ("norm_in", "norm1", "norm2", "norm3"):
                        pack_ln(f"{m}.{n}")
            elif spec.kind == "down":
                wr = f32(pfx + ".op.weight")
                W[pfx + ".w"], W[pfx + ".b"] = pack_conv3x3(dup_k(wr) if "resample" in sp else wr), f32(pfx + ".op.bias")
            elif spec.kind == "up":
                wr = f32(pfx + ".conv.weight")
                if "resample" in sp:  # duplicated along cin, also under the phase operator's taps
                    wr = dup_k(wr)
                W[pfx + ".w"], W[pfx + ".b"] = pack_conv3x3(wr), f32(pfx + ".conv.bias")
                W[pfx + ".w4"] = combine_up_phases(wr)  # ops.conv3x3_up_phases (_resample)
        pack_ln("out.0")
        wh = f32("out.2.weight")
        W["out.2.w"] = pack_conv3x3(dup_k(wh) if "head" in self.split else wh)  # head input [hi | lo] per tap
        W["out.2.b"] = f32("out.2.bias")
        W["emb_all.w"], W["emb_all.b"] = torch.cat(emb_w, 0).contiguous(), torch.cat(emb_b, 0).contiguous()
        W["ctx_all.w"], W["ctx_all.b"] = torch.cat(ctx_w, 0).contiguous(), torch.cat(ctx_b, 0).contiguous()
        self.emb_total, self.ctx_total = emb_total, ctx_total
        self.W = W

    # ------------------------------------------------------------------ helpers
    def _sk(self, rows=0, hw=0, c=0):
        """Workspace of seva_gemm_desc.splitk_ws (one per engine; its launches are serialised on one stream): lets the library run
        the convs of small images (the 9x9 level) as split-K.  `splitk_workspace_numel` of at least 512 tile slots."""
        if not self.conv_splitk:
            return None
        # sized from the launch (never below 512 slots), so that whether a small-image conv is split depends on the per-sample
        # image size only and not on how many samples are batched (a workspace that cannot hold a launch that qualifies for the
        # split is an error in the library, not a fall-back to unsplit tiles: seva_gemm_desc.splitk_ws)
        tiles = max(512, splitk_tiles(rows, c)) if hw and hw <= SPLITK_MAX_PIXELS else 512
        tiles = min(tiles, SPLITK_ERROR_SLOT - 1)
        return self._buf("sk_ws", (splitk_workspace_numel(tiles),), F32, zero=True)

    def _ln(self, x, pfx, rows, c, fp8=False, split=False):
        if split:  # [hi | lo] for duplicated weights
            out = self._buf("ln16s", (rows, 2 * c), F16)
            ops.layernorm_split(x, self.W[pfx + ".g"], self.W[pfx + ".b"], out)
            return out
        if fp8:
            # e4m3 output, K padded to a multiple of 128: the pad columns are zeroed once (nothing ever writes them again)
            out = self._buf("ln8", (rows, _pad128(c)), U8, zero=True)
        else:
            out = self._buf("ln16", (rows, c), F16)
        ops.layernorm(x, self.W[pfx + ".g"], self.W[pfx + ".b"], out)
        return out

    def _slice_rows(self, rows: int, c: int, unit: int) -> int:
        """Rows per pass of a token-wise operator chain (LN -> GEMM -> ... -> GEMM).

        Experiment, off by default (SEVA_SLICE_FRAMES=n enables).  At ds1 the f16 intermediates of one transformer block (LN
        output 139 MB, QKV 418 MB, GEGLU hidden 557 MB) round-trip HBM between producer and consumer; run in slices of a few
        frames through ONE reused slice-sized buffer they could stay in the 256 MB Infinity Cache.  In isolation the GEGLU -> FF2
        pair gains 13 % at 6 frames per slice (927 -> 808 us, tools/kslice.py), but inside the step it does not pay: 105.2 ms
        unsliced vs 105.4 (FF pairs only) / 106.7 ms (whole per-frame attention chain too: the sliced attention launches
        under-fill the chip and the norms shrink).  Results are bitwise unchanged either way (every output row is computed from
        its own input row only; tested).  `unit` = rows that must stay together (a frame)."""
        if self.slice_frames <= 0 or rows * c * 2 < self.slice_min_bytes:
            return rows
        step = self.slice_frames * unit
        return step if step < rows else rows

    def _ff(self, x32, ln_pfx, ff_pfx, rows, c, *, residual, out_f32=None, out_f16=None, unit=1):
        """GEGLU feed-forward on LayerNorm(x32): reference transformer.py:18-34."""
        W = self.W
        if ff_pfx + ".w1f8" in W:
            # fp8 mode, ff="fp8": LayerNorm prologue -> e4m3, GEGLU and FF2 on the scaled fp8 MFMA in ONE kernel
            ops.ff_fused_fp8(None, W[ff_pfx + ".w1f8"], W[ff_pfx + ".w1f8e"], W[ff_pfx + ".b1"], W[ff_pfx + ".w2f8"],
                             W[ff_pfx + ".w2f8e"], W[ff_pfx + ".b2"], residual=residual, out_f32=out_f32, out_f16=out_f16,
                             ln_x=x32, ln_gamma=W[ln_pfx + ".g"], ln_beta=W[ln_pfx + ".b"], ln_eps=1e-5)
            return
        if ff_pfx + ".w18" in W:
            # fp8 chain: LayerNorm -> e4m3, GEGLU on the fp8 MFMA -> e4m3 hidden, FF2 on the fp8 MFMA (+ fp32 residual)
            a8 = self._ln(x32, ln_pfx, rows, c, fp8=True)
            h8 = self._buf("ffh8", (rows, 4 * c), U8)
            ops.gemm(a8, W[ff_pfx + ".w18"], w_exp=W[ff_pfx + ".w18e"], bias=W[ff_pfx + ".b1"], out_f8=h8, geglu=True)
            ops.gemm(h8, W[ff_pfx + ".w28"], w_exp=W[ff_pfx + ".w28e"], bias=W[ff_pfx + ".b2"], residual=residual,
                     out_f32=out_f32, out_f16=out_f16)
            return
        sp_ff = "ff" in self.split
        sp_o16 = out_f16 is not None and "proj_out" in self.split  # out_f16 is `last16`, proj_out's operand
        if sp_ff or sp_o16:
            # split precision: the two-kernel path at every width (the fused kernel has neither a split hidden tensor nor a split out_f16)
            if self._slice_rows(rows, c, unit) < rows:
                raise SevaNativeError("split-precision feed-forwards do not run frame-sliced (SEVA_SLICE_FRAMES)")
            a = self._ln(x32, ln_pfx, rows, c, split=sp_ff)
            hidden = self._buf("ffhs" if sp_ff else "ffh", (rows, (8 if sp_ff else 4) * c), F16)
            (ops.gemm_split_out if sp_ff else ops.gemm)(a, W[ff_pfx + ".w1"], bias=W[ff_pfx + ".b1"], out_f16=hidden, geglu=True,
                                                      alg_k=c if sp_ff else 0)
            (ops.gemm_split_out if sp_o16 else ops.gemm)(hidden, W[ff_pfx + ".w2"], bias=W[ff_pfx + ".b2"], residual=residual,
                                                       out_f32=out_f32, out_f16=out_f16, alg_k=4 * c if sp_ff else 0)
            return
        if self.ff_fused and c in ops.FF_FUSED_CHANNELS:
            # narrow levels (ds1: C = 320): GEGLU -> FF2 in ONE kernel, the 4C-wide hidden tensor never exists in HBM
            # ... and its LayerNorm runs in that kernel's prologue (x32 rows read as fp32, normalised in registers)
            ops.ff_fused(None, W[ff_pfx + ".w1"], W[ff_pfx + ".b1"], W[ff_pfx + ".w2"], W[ff_pfx + ".b2"],
                         residual=residual, out_f32=out_f32, out_f16=out_f16,
                         ln_x=x32, ln_gamma=W[ln_pfx + ".g"], ln_beta=W[ln_pfx + ".b"], ln_eps=1e-5)
            return
        step = self._slice_rows(rows, c, unit)
        a_buf = self._buf("ln16", (step, c), F16)
        h_buf = self._buf("ffh", (step, 4 * c), F16)
        for r0 in range(0, rows, step):
            r1 = min(r0 + step, rows)
            a, hidden = a_buf[: r1 - r0], h_buf[: r1 - r0]
            ops.layernorm(x32[r0:r1], W[ln_pfx + ".g"], W[ln_pfx + ".b"], a)
            ops.gemm(a, W[ff_pfx + ".w1"], bias=W[ff_pfx + ".b1"], out_f16=hidden, geglu=True)
            ops.gemm(hidden, W[ff_pfx + ".w2"], bias=W[ff_pfx + ".b2"],
                     residual=None if residual is None else residual[r0:r1],
                     out_f32=None if out_f32 is None else out_f32[r0:r1],
                     out_f16=None if out_f16 is None else out_f16[r0:r1])

    # ------------------------------------------------------------------ blocks
    def _resblock(self, spec, x1: Act, x2: Act | None, dense, emb_all) -> Act:
        """ResBlock.forward, reference layers.py:120-139.  x1 (‖ x2) fp32 [n, hw, c]."""
        audit_mark(spec.prefix)
        W, pfx = self.W, spec.prefix
        n, h, w, hw = x1.n, x1.h, x1.w, x1.hw
        cin, cout = spec.cin, spec.cout
        f8_1, f8_2 = pfx + ".conv1.w8" in W, pfx + ".conv2.w8" in W  # fp8 mode: the conv consumes e4m3 activations
        sp_conv = "conv" in self.split  # both GroupNorms write [hi | lo] channels, the convs see 2 cin / 2 cout input channels
        k1, k2 = (2 * cin, 2 * cout) if sp_conv else (cin, cout)
        a16 = None if f8_1 else self._buf("gn16", (n, hw, k1), F16)
        cin8, cout8 = _pad128(cin), _pad128(cout)  # fp8 convs see channel counts padded to a multiple of 128 (pad stays zero)
        a8 = self._buf("gn8", (n, hw, cin8), U8, zero=True) if f8_1 else None
        # the 1x1 skip conv (cin != cout) consumes the raw input as f16: emitted by the same GroupNorm pass
        sp_skip = cin != cout and self._split_skip(cout)
        xs16 = self._buf("skip16", (n * hw, (2 if sp_skip else 1) * cin), F16) if cin != cout else None
        self._groupnorm(x1, x2, W[pfx + ".in_layers.0.g"], W[pfx + ".in_layers.0.b"], a16,
                        eps=1e-5, silu=True, dense=dense, dense_w=W[pfx + ".dense.w"], dense_b=W[pfx + ".dense.b"],
                        raw_f16=xs16, out_f8=a8, split_raw=sp_skip, split_out=sp_conv)
        mid = self._out32("res_mid", n, h, w, cout)
        off = self.emb_off[pfx]
        if f8_1:
            ops.conv3x3(a8.view(n, h, w, cin8), W[pfx + ".conv1.w8"], w_exp=W[pfx + ".conv1.w8e"], bias=W[pfx + ".conv1.b"],
                        row_add=emb_all[:, off:], rows_per_group=hw, ld_row_add=self.emb_total, **mid.dst)
        else:
            ops.conv3x3(a16.view(n, h, w, k1), W[pfx + ".conv1.w"], bias=W[pfx + ".conv1.b"],
                        row_add=emb_all[:, off:], rows_per_group=hw, ld_row_add=self.emb_total, **mid.dst,
                        splitk_ws=self._sk(n * hw, hw, cout), alg_k=9 * cin if sp_conv else 0)
        b16 = None if f8_2 else self._buf("gn16", (n, hw, k2), F16)
        b8 = self._buf("gn8", (n, hw, cout8), U8, zero=True) if f8_2 else None
        self._groupnorm(mid, None, W[pfx + ".out_layers.0.g"], W[pfx + ".out_layers.0.b"], b16,
                        eps=1e-5, silu=True, out_f8=b8, split_out=sp_conv)
        fold = cin != cout and self.fold_skip and not f8_2 and (hw > 128 or not self.conv_splitk)
        if fold:
            res = None
        elif cin != cout:
            res = self._buf("skip32", (n * hw, cout), F32)
            ops.gemm(xs16, W[pfx + ".skip.w"], bias=W[pfx + ".skip.b"], out_f32=res, alg_k=cin)  # ([hi | lo] doubles K, not the FLOP credit)
        else:
            assert x2 is None
            res = x1.t
        out = self._out32("out:" + pfx, n, h, w, cout)
        if fold:
            ops.conv3x3(b16.view(n, h, w, k2), W[pfx + ".conv2.wf"], bias=W[pfx + ".conv2.bf"], a2=xs16, **out.dst)
        elif f8_2:
            ops.conv3x3(b8.view(n, h, w, cout8), W[pfx + ".conv2.w8"], w_exp=W[pfx + ".conv2.w8e"], bias=W[pfx + ".conv2.b"],
                        residual=res, **out.dst)
        else:
            ops.conv3x3(b16.view(n, h, w, k2), W[pfx + ".conv2.w"], bias=W[pfx + ".conv2.b"],
                        residual=res, **out.dst, splitk_ws=self._sk(n * hw, hw, cout),
                        alg_k=9 * cout if sp_conv else 0)
        return out

    def _self_attention(self, x32, ln_pfx, at_pfx, rows, c, heads, *, regime, n, hw, T, residual,
                        row_add, rpg, ldra, out_f32):
        """Attention.forward (self), reference transformer.py:59-74, + residual (+ folded attn2)."""
        W = self.W
        c3 = 3 * c
        sp_qkv = "qkv" in self.split  # the LayerNorm output travels as [hi | lo]; q / k / v themselves stay f16
        if sp_qkv and regime == "frame" and self.slice_attn and self._slice_rows(rows, c, hw) < rows:
            raise SevaNativeError("the split-precision QKV projection does not run frame-sliced (SEVA_SLICE_ATTN)")
        if regime == "frame" and self.slice_attn and self._slice_rows(rows, c, hw) < rows:
            # per-frame attention: the whole chain LN -> QKV -> attention -> out-projection runs a few frames at a time
            step = self._slice_rows(rows, c, hw)
            a_buf = self._buf("ln16", (step, c), F16)
            qkv_buf = self._buf("qkv", (step, c3), F16)
            att_buf = self._buf("att", (step, c), F16)
            for r0 in range(0, rows, step):
                r1 = min(r0 + step, rows)
                nr, f0, nf = r1 - r0, r0 // hw, (r1 - r0) // hw
                a, qkv, att = a_buf[:nr], qkv_buf[:nr], att_buf[:nr]
                ops.layernorm(x32[r0:r1], W[ln_pfx + ".g"], W[ln_pfx + ".b"], a)
                ops.gemm(a, W[at_pfx + ".qkv"], out_f16=qkv, col_scale=QK_SCALE_LOG2E, col_scale_n=c)
                ops.attention(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], att, nb0=nf, nb1=1, heads=heads, lq=hw, lk=hw,
                              q_strides=(hw * c3, 0, c3), k_strides=(hw * c3, 0, c3), o_strides=(hw * c, 0, c),
                              q_prescaled=True)
                ops.gemm(att, W[at_pfx + ".out.w"], bias=W[at_pfx + ".out.b"], residual=residual[r0:r1],
                         row_add=None if row_add is None else row_add[f0:], rows_per_group=rpg, ld_row_add=ldra,
                         out_f32=out_f32[r0:r1])
            return
        qkv = self._buf("qkv", (rows, 3 * c), F16)
        # softmax scale * log2(e) rides on the q third of the projection (fp32, before the single f16
        # rounding), so the attention kernel exponentiates its MFMA output directly
        if at_pfx + ".qkv8" in W:  # fp8 mode: e4m3 LayerNorm output x e4m3 weights, f16 q/k/v out
            a8 = self._ln(x32, ln_pfx, rows, c, fp8=True)
            ops.gemm(a8, W[at_pfx + ".qkv8"], w_exp=W[at_pfx + ".qkv8e"], out_f16=qkv, col_scale=QK_SCALE_LOG2E, col_scale_n=c)
        else:
            a = self._ln(x32, ln_pfx, rows, c, split=sp_qkv)
            ops.gemm(a, W[at_pfx + ".qkv"], out_f16=qkv, col_scale=QK_SCALE_LOG2E, col_scale_n=c, alg_k=c if sp_qkv else 0)
        att = self._buf("att", (rows, c), F16)
        q, k, v = qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:]
        if regime == "frame":  # batch = frame, tokens = pixels
            self._attention_long(q, k, v, att, nb0=n, heads=heads, L=hw, q_strides=(hw * c3, 0, c3),
                                 k_strides=(hw * c3, 0, c3), o_strides=(hw * c, 0, c), split_ws=None)
        elif regime == "joint":  # batch = scene, tokens = (frame, pixel)
            # long key sequences (L = T hw >= ops.ATTN_SPLIT_MIN_LK) run K/V-split: the workspace for the two partial results
            sws = None
            if self.attn_split and T * hw >= ops.ATTN_SPLIT_MIN_LK:
                sws = self._buf("attn_split", (ops.attention_split_workspace_numel(n // T, heads, T * hw, self.attn_split_max),), F32)
            self._attention_long(q, k, v, att, nb0=n // T, heads=heads, L=T * hw, q_strides=(T * hw * c3, 0, c3),
                                 k_strides=(T * hw * c3, 0, c3), o_strides=(T * hw * c, 0, c), split_ws=sws)
        else:  # temporal: batch = (scene, pixel), tokens = frames, read through strides
            ops.attention(q, k, v, att, nb0=n // T, nb1=hw, heads=heads, lq=T, lk=T,
                          q_strides=(T * hw * c3, c3, hw * c3), k_strides=(T * hw * c3, c3, hw * c3),
                          o_strides=(T * hw * c, c, hw * c), q_prescaled=True)
        ops.gemm(att, W[at_pfx + ".out.w"], bias=W[at_pfx + ".out.b"], residual=residual,
                 row_add=row_add, rows_per_group=rpg, ld_row_add=ldra, out_f32=out_f32)

    def _attention_long(self, q, k, v, att, *, nb0, heads, L, q_strides, k_strides, o_strides, split_ws):
        """Per-frame / joint self-attention (q pre-scaled).  fp8 attention sub-option: the launches of L >= ops.PV8_MIN_LQ (those
        seva_attention_f16 runs on attn16_kernel) quantise V into an arena workspace and take seva_attention_pv8."""
        if self.pv8 and L >= ops.PV8_MIN_LQ:
            ws = self._buf("v_fp8", (ops.v_fp8_workspace_numel(nb0, heads, L),), U8)
            ops.quantize_v_fp8(v, ws, nb0=nb0, nb1=1, heads=heads, lk=L, k_strides=k_strides)
            ops.attention_pv8(q, k, ws, att, nb0=nb0, nb1=1, heads=heads, lq=L, lk=L, q_strides=q_strides,
                              k_strides=k_strides, o_strides=o_strides, split_ws=split_ws)
            return
        ops.attention(q, k, v, att, nb0=nb0, nb1=1, heads=heads, lq=L, lk=L, q_strides=q_strides, k_strides=k_strides,
                      o_strides=o_strides, q_prescaled=True, split_ws=split_ws)

    def _cross_attention_general(self, x32, ln_pfx, at_pfx, rows, c, heads, ctx16, lc, *, nb0, nb1,
                                 lq, q_strides, o_strides, ctx_batch_stride, out_f32):
        """Attention.forward with a context of length > 1 (reference transformer.py:59-74)."""
        W = self.W
        a = self._ln(x32, ln_pfx, rows, c)
        q = self._buf("xq", (rows, c), F16)
        ops.gemm(a, W[at_pfx + ".q"], out_f16=q)
        kv = self._buf("xkv", (ctx16.shape[0], 2 * c), F16)
        ops.gemm(ctx16, W[at_pfx + ".kv"], out_f16=kv)
        att = self._buf("att", (rows, c), F16)
        ops.attention(q, kv[:, :c], kv[:, c:], att, nb0=nb0, nb1=nb1, heads=heads, lq=lq, lk=lc,
                      q_strides=q_strides, k_strides=(ctx_batch_stride * 2 * c, 0, 2 * c),
                      o_strides=o_strides)
        ops.gemm(att, W[at_pfx + ".out.w"], bias=W[at_pfx + ".out.b"], residual=x32, out_f32=out_f32)

    def _transformer(self, spec, x: Act, T, ctxvec, ctx16, lc) -> Act:
        """MultiviewTransformer.forward, reference transformer.py:215-247."""
        audit_mark(spec.prefix)
        W, pfx, c, heads = self.W, spec.prefix, spec.channels, spec.heads
        n, hw, rows = x.n, x.hw, x.rows
        sp_in, sp_out = "proj_in" in self.split, "proj_out" in self.split
        cs = 2 * c if sp_in else c
        g16 = self._buf("gn16", (n, hw, cs), F16)
        self._groupnorm(x, None, W[pfx + ".norm.g"], W[pfx + ".norm.b"], g16, eps=1e-6, silu=False, split_out=sp_in)
        cur = self._buf("t_h", (rows, c), F32)
        ops.gemm(g16.view(rows, cs), W[pfx + ".proj_in.w"], bias=W[pfx + ".proj_in.b"], out_f32=cur, alg_k=c if sp_in else 0)
        collapse = lc == 1
        ldra_frame, ldra_scene = self.ctx_total, T * self.ctx_total
        last16 = None
        for i in range(spec.depth):
            b = f"{pfx}.transformer_blocks.{i}"
            m = f"{pfx}.time_mix_blocks.{i}"
            regime = "joint" if spec.joint else "frame"
            audit_mark(b)
            # x = attn1(norm1 x) + x ; x = attn2(norm2 x, ctx) + x
            h1 = self._buf("t_h1", (rows, c), F32)
            if collapse:
                ra = ctxvec[:, self.ctx_off[b + ".attn2"]:]
                rpg, ldra = (T * hw, ldra_scene) if spec.joint else (hw, ldra_frame)
                self._self_attention(cur, b + ".norm1", b + ".attn1", rows, c, heads, regime=regime, n=n,
                                     hw=hw, T=T, residual=cur, row_add=ra, rpg=rpg, ldra=ldra, out_f32=h1)
            else:
                h0 = self._buf("t_h0", (rows, c), F32)
                self._self_attention(cur, b + ".norm1", b + ".attn1", rows, c, heads, regime=regime, n=n,
                                     hw=hw, T=T, residual=cur, row_add=None, rpg=0, ldra=0, out_f32=h0)
                if spec.joint:  # context[::T], one per scene
                    self._cross_attention_general(
                        h0, b + ".norm2", b + ".attn2", rows, c, heads, ctx16, lc, nb0=n // T, nb1=1,
                        lq=T * hw, q_strides=(T * hw * c, 0, c), o_strides=(T * hw * c, 0, c),
                        ctx_batch_stride=T * lc, out_f32=h1)
                else:
                    self._cross_attention_general(
                        h0, b + ".norm2", b + ".attn2", rows, c, heads, ctx16, lc, nb0=n, nb1=1, lq=hw,
                        q_strides=(hw * c, 0, c), o_strides=(hw * c, 0, c), ctx_batch_stride=lc, out_f32=h1)
            # x = ff(norm3 x) + x
            h2 = self._buf("t_h2", (rows, c), F32)
            self._ff(h1, b + ".norm3", b + ".ff", rows, c, residual=h1, out_f32=h2, unit=hw)
            # ---- time-mix block on x_spatial = h2 (transformer.py:145-155) ----
            audit_mark(m)
            m1 = self._buf("t_m1", (rows, c), F32)
            self._ff(h2, m + ".norm_in", m + ".ff_in", rows, c, residual=h2, out_f32=m1, unit=hw)
            m2 = self._buf("t_m2", (rows, c), F32)
            if collapse:
                ra = ctxvec[:, self.ctx_off[m + ".attn2"]:]
                self._self_attention(m1, m + ".norm1", m + ".attn1", rows, c, heads, regime="temporal", n=n,
                                     hw=hw, T=T, residual=m1, row_add=ra, rpg=T * hw, ldra=ldra_scene, out_f32=m2)
            else:
                m0 = self._buf("t_m0", (rows, c), F32)
                self._self_attention(m1, m + ".norm1", m + ".attn1", rows, c, heads, regime="temporal", n=n,
                                     hw=hw, T=T, residual=m1, row_add=None, rpg=0, ldra=0, out_f32=m0)
                self._cross_attention_general(
                    m0, m + ".norm2", m + ".attn2", rows, c, heads, ctx16, lc, nb0=n // T, nb1=hw, lq=T,
                    q_strides=(T * hw * c, c, hw * c), o_strides=(T * hw * c, c, hw * c),
                    ctx_batch_stride=T * lc, out_f32=m2)
            # x = x_spatial + ff(norm3 x_mix)   (time-mix ff has no residual; SkipConnect adds)
            final = i == spec.depth - 1
            nxt = None if final else self._buf("t_h", (rows, c), F32)
            last16 = self._buf("t_h16", (rows, 2 * c if sp_out else c), F16)  # (split: [hi | lo], written by _ff's FF2)
            self._ff(m2, m + ".norm3", m + ".ff", rows, c, residual=h2, out_f32=nxt, out_f16=last16, unit=hw)
            cur = nxt
        audit_mark(pfx)
        out = self._out32("out:" + pfx, n, x.h, x.w, c)
        ops.gemm(last16, W[pfx + ".proj_out.w"], bias=W[pfx + ".proj_out.b"], residual=x.t2, **out.dst2, alg_k=c if sp_out else 0)
        return out

    def _resample(self, spec, x: Act) -> Act:
        """Downsample (layers.py:49-58) / Upsample (layers.py:35-46)."""
        audit_mark(spec.prefix)
        c = spec.channels
        n, h, w = x.n, x.h, x.w
        sp_rs = "resample" in self.split
        x16 = self._buf("rs16", (n, h, w, 2 * c if sp_rs else c), F16)
        (ops.cast_concat_f16_split if sp_rs else ops.cast_concat_f16)(x.t, None, x16)
        alg_k = 9 * c if sp_rs else 0
        if spec.kind == "down":
            oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            out = self._out32("out:" + spec.prefix, n, oh, ow, c)
            ops.conv3x3(x16, self.W[spec.prefix + ".w"], stride=2, bias=self.W[spec.prefix + ".b"], **out.dst,
                        splitk_ws=self._sk(n * oh * ow, oh * ow, c), alg_k=alg_k)
            return out
        oh, ow = 2 * h, 2 * w
        phases = getattr(ops, "conv3x3_up_phases", None)
        if phases is not None and c % 160 == 0 and env_flag("SEVA_UPSAMPLE_PHASES", "not0", True):  # (read at every call)
            # four 2x2 phase convs on the source image: 4/9 of the FLOPs.  The path emits no statistics (a 64-row block of one
            # phase is not image-aligned), so the consuming GroupNorm runs its own pass over this tensor
            out = Act(self._buf("out:" + spec.prefix, (n, oh * ow, c), F32), n, oh, ow)
            phases(x16, self.W[spec.prefix + ".w4"], bias=self.W[spec.prefix + ".b"], **out.dst, alg_k=9 * c)
        else:
            out = self._out32("out:" + spec.prefix, n, oh, ow, c)
            ops.conv3x3(x16, self.W[spec.prefix + ".w"], upsample=True, bias=self.W[spec.prefix + ".b"], **out.dst, alg_k=alg_k)
        return out

    # ------------------------------------------------------------------ graph replay
    @torch.no_grad()
    def forward_graphed(self, x, concat, t, y, dense_y, num_frames, shallow_levels=0):
        """Same result as `forward`, replayed from a hipGraph.  First call of a signature runs eagerly
        twice (arena warm-up, then capture on a side stream); later calls copy the inputs into the
        static buffers and launch the instantiated graph: one launch instead of ~550.  A shallow call has a graph of its
        own per signature and depth, and passes the same guard as an eager one before every replay."""
        require_cuda(x, t, y, dense_y)
        if concat is not None and concat.numel() == 0:
            concat = None
        L = int(shallow_levels)
        sig = self._signature(x, concat, y, dense_y, num_frames)
        if L:
            self._shallow_entry(L, sig)
        key = sig + (L,)
        fwd = lambda *a, **k: self.forward(*a, shallow_levels=L, **k)  # noqa: E731
        ent = self._graphs.get(key)
        if ent is None:
            # static input buffers: ordinary tensors even under torch.inference_mode() (reference eval.py:1242) -- an
            # inference tensor could not be refreshed in place by a later call made outside that mode
            with torch.inference_mode(False):
                st = {
                    "x": torch.empty(x.shape, dtype=F32, device=self.device),
                    "concat": None if concat is None else torch.empty(concat.shape, dtype=F32, device=self.device),
                    "t": torch.empty(t.shape, dtype=torch.int64, device=self.device),
                    "y": torch.empty(y.shape, dtype=F32, device=self.device),
                    "dense": torch.empty(dense_y.shape, dtype=F32, device=self.device),
                }
                out = torch.empty((x.shape[0], self.p.out_channels) + tuple(x.shape[2:]), dtype=F32, device=self.device)
            self._copy_inputs(st, x, concat, t, y, dense_y)
            fwd(st["x"], st["concat"], st["t"], st["y"], st["dense"], num_frames, out=out)  # warm the arena
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            graph = ops.Graph()
            with torch.cuda.stream(side):
                graph.capture_begin(self.device)
                try:
                    fwd(st["x"], st["concat"], st["t"], st["y"], st["dense"], num_frames, out=out)
                except BaseException:
                    # leave no stream stuck in capture mode: end + discard the partial graph, then run eagerly from now on
                    try:
                        graph.capture_end(self.device)
                    except Exception:
                        pass
                    self.use_graph = False
                    raise
                graph.capture_end(self.device)
            torch.cuda.current_stream(self.device).wait_stream(side)
            ent = (graph, st, out)
            self._graphs[key] = ent
        graph, st, out = ent
        self._copy_inputs(st, x, concat, t, y, dense_y)
        if not L:
            self._last_full = None
        graph.launch(self.device)
        if not L:  # the replay refilled the buffers that this signature's capture recorded as entry points
            self._last_full = sig
        return out.clone()

    @staticmethod
    def _copy_inputs(st, x, concat, t, y, dense_y):
        st["x"].copy_(x)
        if st["concat"] is not None:
            st["concat"].copy_(concat)
        st["t"].copy_(t)
        st["y"].copy_(y)
        st["dense"].copy_(dense_y)

    @audit.first_call
    def __call__(self, x, concat, t, y, dense_y, num_frames):
        # inside a whole-step capture (seva/_stepgraph.py) or its warm-up the network is launched eagerly: its ~600
        # kernels become nodes of the step graph instead of a nested replay
        L = _native.network_shallow_levels()  # (`_native.shallow_network`: the sampler's request for a shallow call)
        if self.use_graph and not _native.network_eager_forced() and not torch.cuda.is_current_stream_capturing():
            return self.forward_graphed(x, concat, t, y, dense_y, num_frames, shallow_levels=L)
        return self.forward(x, concat, t, y, dense_y, num_frames, shallow_levels=L)

    # ------------------------------------------------------------------ shallow calls
    @staticmethod
    def _signature(x, concat, y, dense_y, num_frames) -> tuple:
        """What two calls must share for one to reuse the other's buffers (also the key of `forward_graphed`'s graphs)."""
        return (tuple(x.shape), None if concat is None or concat.numel() == 0 else tuple(concat.shape), tuple(y.shape),
                tuple(dense_y.shape), int(num_frames))

    def shallow_input_blocks(self, levels: int) -> int:
        """m: a shallow call of depth `levels` runs the m input blocks after the stem that precede the `levels`-th Downsample of
        the layout, and the last m + 1 output blocks (2 / 5 / 8 for the 1.3 B architecture)."""
        if not 1 <= levels <= len(self._shallow_m):
            raise ValueError(f"shallow_levels must be 0 (a full call) or 1..{len(self._shallow_m)}, got {levels!r}")
        return self._shallow_m[levels - 1]

    def _shallow_entry(self, levels: int, sig: tuple):
        """The guard of a shallow call: the `Act` (tensor and statistics) that the last full call left for depth `levels`, or
        SevaNativeError when that call was not one of this signature -- never a buffer the engine cannot vouch for."""
        self.shallow_input_blocks(levels)
        last = self._last_full
        if last is None:
            raise SevaNativeError(
                f"shallow network call (shallow_levels={levels}): this engine has made no full call to reuse (an engine built anew, "
                "as after set_precision or a weight reload, starts without one, and so does one whose last full call failed)")
        if last != sig:
            names = ("x", "concat", "y", "dense_y", "num_frames")
            diff = ", ".join(f"{k} {a} -> {b}" for k, a, b in zip(names, last, sig) if a != b)
            raise SevaNativeError(f"shallow network call (shallow_levels={levels}): the last full call had another signature ({diff})")
        return self._shallow_entries[sig][levels]

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, x, concat, t, y, dense_y, num_frames, out=None, shallow_levels=0):
        """x: [n, c, h, w] f32 (‖ concat on channels), t: [n] int64 sigma indices, y: [n, L, ctx],
        dense_y: [n, 6, hd, wd].  Returns [n, out_channels, h, w] f32.

        shallow_levels = L in 1..3 (opt-in; DESIGN.md section 5, "Reuse of deep features"): run only the prologue, the stem, the
        input blocks above the L-th Downsample, the matching last output blocks and the head; what enters the first of those
        output blocks is the tensor (and its GroupNorm statistics) that the most recent full call of the same signature left
        in the arena.  Without such a call: SevaNativeError (`_shallow_entry`), never a silent full call."""
        require_cuda(x, t, y, dense_y)
        W, p, lay = self.W, self.p, self.layout
        x = x.to(F32).contiguous()
        concat = None if concat is None or concat.numel() == 0 else concat.to(F32).contiguous()
        dense_y = dense_y.to(F32).contiguous()
        n, cx, h, w = x.shape
        T = int(num_frames)
        cin = cx + (concat.shape[1] if concat is not None else 0)
        if cin != p.in_channels:
            raise ValueError(f"expected {p.in_channels} input channels, got {cin}")
        if n % T:
            raise ValueError(f"batch {n} is not a multiple of num_frames {T}")
        assert y.ndim == 3
        lc = y.shape[1]
        t = t.to(torch.int64).contiguous()
        L = int(shallow_levels)
        sig = self._signature(x, concat, y, dense_y, T)
        if L:
            entry = self._shallow_entry(L, sig)
            m_in = self.shallow_input_blocks(L)
        else:
            self._last_full = None  # (until this call has run to its end)
            entries: dict = {}
            enters = {m + 1: k + 1 for k, m in enumerate(self._shallow_m)}  # output blocks left to run -> the depth that enters there
        self.gn_ws = self._buf("gn_ws", (n * ops.GN_WORKSPACE_SLABS * 32 * 2,), F32)

        # --- prologue: timestep embedding MLP, all ResBlock emb projections, folded cross-attn ---
        audit_mark("time_embed")
        mc, ed = p.model_channels, lay.time_embed_dim
        te16 = self._buf("te16", (n, mc), F16)
        ops.timestep_embedding_f16(t, W["freqs"], te16)
        e1 = self._buf("te_h", (n, ed), F32)
        ops.gemm(te16, W["time_embed.0.w"], bias=W["time_embed.0.b"], out_f32=e1)
        e1a = self._buf("te_h16", (n, ed), F16)
        ops.silu_f16(e1, e1a)
        emb = self._buf("emb", (n, ed), F32)
        ops.gemm(e1a, W["time_embed.2.w"], bias=W["time_embed.2.b"], out_f32=emb)
        emb_a = self._buf("emb16", (n, ed), F16)
        ops.silu_f16(emb, emb_a)
        emb_all = self._buf("emb_all", (n, self.emb_total), F32)
        ops.gemm(emb_a, W["emb_all.w"], bias=W["emb_all.b"], out_f32=emb_all)
        ctx16 = self._buf("ctx16", (n * lc, y.shape[2]), F16)
        ops.cast_concat_f16(y.to(F32).contiguous().view(n * lc, -1), None, ctx16)
        ctxvec = None
        if lc == 1:
            ctxvec = self._buf("ctxvec", (n, self.ctx_total), F32)
            ops.gemm(ctx16, W["ctx_all.w"], bias=W["ctx_all.b"], out_f32=ctxvec)

        dense_cache: dict = {}

        def dense_at(hh, ww):
            key = (hh, ww)
            if key not in dense_cache:
                d = self._buf("dense", (n, hh * ww, dense_y.shape[1]), F32)
                ops.bilinear_to_nhwc(dense_y, d, hh, ww)
                dense_cache[key] = d
            return dense_cache[key]

        # --- stem ---
        stem = lay.input_blocks[0][0]
        audit_mark(stem.prefix)
        sp_stem = "stem" in self.split and 2 * cin <= CIN_PAD
        cpad = CIN_PAD * (((2 if sp_stem else 1) * cin + CIN_PAD - 1) // CIN_PAD)
        x16 = self._buf("x16", (n, h, w, cpad), F16)
        ops.nchw_to_nhwc_f16(x, concat, x16, split=sp_stem)
        cur = self._out32("out:" + stem.prefix, n, h, w, stem.cout)
        ops.conv3x3(x16, W[stem.prefix + ".w"], bias=W[stem.prefix + ".b"], **cur.dst,
                    alg_k=9 * cin)  # (profiling counts the reference's 11 input channels, not the padded / split 64)
        hs = [cur]

        def run(block, cur, x2):
            for spec in block:
                if spec.kind == "res":
                    cur = self._resblock(spec, cur, x2, dense_at(cur.h, cur.w), emb_all)
                    x2 = None
                elif spec.kind == "mvt":
                    cur = self._transformer(spec, cur, T, ctxvec, ctx16, lc)
                else:
                    cur = self._resample(spec, cur)
            return cur

        nout = len(lay.output_blocks)
        for block in lay.input_blocks[1:1 + m_in] if L else lay.input_blocks[1:]:
            cur = run(block, cur, None)
            hs.append(cur)
        cur = entry if L else run(lay.middle, cur, None)  # (a reused tensor arrives with its producer's statistics)
        for k in range(nout - (m_in + 1) if L else 0, nout):
            if not L and nout - k in enters:
                entries[enters[nout - k]] = cur
            skip = hs.pop()
            assert (skip.h, skip.w) == (cur.h, cur.w)
            cur = run(lay.output_blocks[k], cur, skip)
        assert not hs

        # --- head: GroupNorm + SiLU + conv3x3 (model.py:170-174) ---
        audit_mark("out")
        cfin = lay.final_channels
        sp_head = "head" in self.split
        cf2 = (2 if sp_head else 1) * cfin
        g16 = self._buf("gn16", (n, cur.hw, cf2), F16)
        self._groupnorm(cur, None, W["out.0.g"], W["out.0.b"], g16, eps=1e-5, silu=True, split_out=sp_head)
        o_nhwc = self._buf("head", (n, cur.hw, p.out_channels), F32)
        ops.conv3x3(g16.view(n, cur.h, cur.w, cf2), W["out.2.w"], bias=W["out.2.b"], out_f32=o_nhwc, alg_k=9 * cfin)
        if out is None:
            out = torch.empty((n, p.out_channels, cur.h, cur.w), dtype=F32, device=self.device)
        ops.nhwc_to_nchw_f32(o_nhwc, out)
        if not L:
            self._shallow_entries[sig] = entries
            self._last_full = sig
        return out
