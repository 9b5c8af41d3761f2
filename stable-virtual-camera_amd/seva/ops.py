"""Tensor-level wrappers over the C-ABI operators of libseva_hip.so.

Every function enqueues HIP kernels on PyTorch's current stream through raw device pointers;
PyTorch is used for memory and streams only.  Outputs are caller-provided (graph-capture
friendly: no allocation happens here unless `out=None`).  Layouts follow include/seva_hip.h:
channels-last activations, f16 GEMM operands, f32 residual stream.
"""

from __future__ import annotations

import ctypes as C
import functools
import inspect

import torch

from . import _native as nv
from ._native import AttnDesc, GemmDesc, GroupNormDesc, ImageDesc, LpipsLayerDesc, MetricsDesc, check, ptr, require_cuda, stream_ptr

F16, F32 = torch.float16, torch.float32
U8 = torch.uint8  # e4m3 bytes travel as uint8 tensors (bit pattern of torch.float8_e4m3fn)


def _lib():
    return nv.load()


# --- dynamic-range audit (seva/audit.py; the kernel's contract is in include/seva_hip.h) --------------------------------
RANGE_WORDS = 72         # SEVA_RANGE_WORDS
RANGE_WG_ELEMS = 32768   # SEVA_RANGE_WG_ELEMS: elements one workgroup of the counting kernel takes (tensors up to RANGE_MAX_WGS of them)
RANGE_MAX_WGS = 2048     # SEVA_RANGE_MAX_WGS: most workgroups (partial tables) of the counting kernel
RANGE_DTYPES = {F32: 0, F16: 1, U8: 2}  # SEVA_RANGE_F32 / _F16 / _E4M3

# wrapper name -> names of its floating-point (f32 / f16 / e4m3) output parameters; filled by `_audited`.  While a recorder is
# active (`audit.record()`), a listed wrapper hands each output it was given to the recorder after its launch.
AUDITED: dict = {}
# every other function of this module that calls the library, and why its outputs are not audited
NOT_AUDITED = {
    "tensor_range": "the audit's own instrument (uint64 words)",
    "tensor_range_workspace_numel": "size query",
    "_up_phases": "shared body of conv3x3_up_phases / conv3x3_up_phases128, which are audited",
    "_v_fp8_parts": "size query",
    "rgb_to_u8": "uint8 output",
    "frame_metrics_workspace_numel": "size query",
    "frame_metrics": "integer and fp64 sums",
    "lpips_layer_workspace_numel": "size query",
    "lpips_layer": "fp64 sums",
    "set_knob": "knob",
    "get_knob": "knob",
    "last_plan": "plan name of the last launch",
    "prof_enable": "profiling switch",
    "prof_collect": "profiling counters",
}
_AUDIT = None  # the active recorder (seva.audit.Recorder), None = off: the wrappers then do exactly what they did before


def audit_mark(scope: str) -> None:
    """Name the part of the network the following launches belong to (a state-dict prefix), until the next mark.  A no-op
    unless a recorder is active."""
    if _AUDIT is not None:
        _AUDIT.scope = scope


def _audited(*outputs: str):
    def deco(fn):
        AUDITED[fn.__name__] = outputs
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def wrapper(*a, **kw):
            if _AUDIT is None:
                return fn(*a, **kw)
            r = fn(*a, **kw)
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            audit_outputs(fn.__name__, bound.arguments)
            return r

        return wrapper

    return deco


def audit_outputs(op: str, a: dict) -> None:
    """Hand the outputs of one call of wrapper `op` (a: its arguments by name) to the active recorder."""
    if _AUDIT is None:
        return
    for name in AUDITED[op]:
        t = a.get(name)
        if t is not None:
            for label, off, rows, cols, pitch in _audit_views(op, name, t, a):
                _AUDIT.output(op, label, t, off, rows, cols, pitch)


def _as_2d(t: torch.Tensor) -> list:
    """(element offset, rows, cols, pitch) pieces that cover exactly the elements of `t` (unit inner stride)."""
    if t.dim() == 0 or t.numel() == 0:
        return [] if t.numel() == 0 else [(0, 1, 1, 1)]
    assert t.stride(-1) == 1 or t.shape[-1] == 1, "audited outputs have unit inner stride"
    shape, stride = list(t.shape), list(t.stride())
    cols, j = 1, len(shape) - 1
    while j >= 0 and (shape[j] == 1 or stride[j] == cols):  # the dense tail
        cols *= shape[j]
        j -= 1
    if j < 0:
        return [(0, t.numel() // shape[-1], shape[-1], shape[-1])]
    if all(shape[i + 1] == 1 or stride[i] == stride[i + 1] * shape[i + 1] for i in range(j)):  # one pitch above the tail
        rows = 1
        for i in range(j + 1):
            rows *= shape[i]
        return [(0, rows, cols, stride[j])]
    return [(i * stride[0] + o, r, c, p) for i in range(shape[0]) for o, r, c, p in _as_2d(t[i])]


def _audit_views(op: str, name: str, t: torch.Tensor, a: dict) -> list:
    """(label, element offset, rows, cols, pitch) records of output `name` of wrapper `op`: the logical area the launch wrote.
    A split-precision [hi | lo] output is two records."""
    def lastdim(cols, split=False, rows=None):
        rows = t.numel() // t.shape[-1] if rows is None else rows
        pitch = t.stride(-2) if t.dim() >= 2 else t.shape[-1]
        if split:
            return [(name + ".hi", 0, rows, cols, pitch), (name + ".lo", cols, rows, cols, pitch)]
        return [(name, 0, rows, cols, pitch)]

    if op == "gemm":
        no = a["w"].shape[0] // (2 if a["geglu"] else 1)
        return lastdim(no, split=a["split_out"] and name == "out_f16", rows=a["a"].shape[0])
    if op == "conv3x3":
        return lastdim(a["w"].shape[0])
    if op in ("conv3x3_up_phases", "conv3x3_up_phases128"):
        return lastdim(a["w4"].shape[1])
    if op in ("ff_fused", "ff_fused_fp8"):
        return lastdim(a["w2"].shape[0])
    if op == "groupnorm":
        c = a["x1"].shape[2] + (a["x2"].shape[2] if a["x2"] is not None else 0)
        return lastdim(c, split=(name == "out_f16" and a["split_out"]) or (name == "raw_f16" and a["split_raw"]),
                       rows=a["x1"].shape[0] * a["x1"].shape[1])
    if op == "layernorm":
        c = a["x"].shape[-1]
        return lastdim(c, rows=a["x"].numel() // c)
    if op in ("layernorm_split", "cast_concat_f16_split"):
        return lastdim(t.shape[-1] // 2, split=True)
    if op == "nchw_to_nhwc_f16":  # (the pad channels behind them are zeros, not values)
        return lastdim(a["x1"].shape[1] + (a["x2"].shape[1] if a["x2"] is not None else 0), split=a["split"])
    if op == "softmax_rows":  # (likewise the zero columns from `cols` up)
        return lastdim(a["cols"])
    if op == "clip_preprocess":
        return lastdim(3 * a["patch"] * a["patch"])
    if op == "quantize_v_fp8":  # the e4m3 values; the E8M0 scale bytes behind them are no e4m3 numbers
        return [(name, 0, 1, _v_fp8_parts(a["nb0"] * a["nb1"], a["heads"], a["lk"])[0], t.numel())]
    return [(name, off, rows, cols, pitch) for off, rows, cols, pitch in _as_2d(t)]


def _size_query(fn, *dims: int) -> int:
    """what a `seva_*_size(dims..., &bytes)` query of the library reports"""
    size = C.c_int64()
    check(fn(*(int(d) for d in dims), C.byref(size)), fn.__name__)
    return size.value


def _workspace(workspace: torch.Tensor | None, need: int, device, who: str) -> torch.Tensor:
    """the caller's uint8 workspace, checked against `need` elements; None: allocated here"""
    if workspace is None:
        workspace = torch.empty(need, dtype=U8, device=device)
    assert workspace.dtype == U8 and workspace.is_contiguous() and workspace.numel() >= need, f"{who} workspace too small"
    return workspace


def _dense_planes(x: torch.Tensor, what: str) -> None:
    H, W = x.shape[2:]
    assert x.stride(3) == 1 and x.stride(2) == W and x.stride(1) == H * W, f"{what} planes must be dense"


def _frame_layout(x: torch.Tensor) -> tuple[int, int, int, int]:
    """(kind, n, H, W) of a frame batch: the ABI's kind 0 = uint8 (n,H,W,3), dense images, 1 = fp32 (n,3,H,W), dense planes; any image pitch"""
    if x.dtype == U8:
        n, H, W, c = x.shape
        assert c == 3 and x.stride(3) == 1 and x.stride(2) == 3 and x.stride(1) == 3 * W, "uint8 frames: (n,H,W,3) with dense images"
        return 0, n, H, W
    n, c, H, W = x.shape
    assert c == 3 and x.stride(3) == 1 and x.stride(2) == W and x.stride(1) == H * W, "fp32 frames: (n,3,H,W) with dense planes"
    return 1, n, H, W


def tensor_range_workspace_numel(rows: int, cols: int) -> int:
    """uint8 elements of `tensor_range(workspace=...)`: one 72-word partial table per workgroup of the counting kernel."""
    return _size_query(_lib().seva_tensor_range_size, rows, cols)


def tensor_range(x: torch.Tensor, out: torch.Tensor | None = None, *, rows: int | None = None, cols: int | None = None,
                 workspace: torch.Tensor | None = None) -> torch.Tensor:
    """Exponent histogram, special-value counts and finite extrema of x in one pass (seva_tensor_range; the 72-word contract is in
    include/seva_hip.h).  x: a 2-D view (or 1-D: one row) with unit inner stride, f32, f16, or uint8 = e4m3 bytes; rows / cols
    narrow the audited area to its top-left corner.  Returns `out`: 72 uint64 words on the device, held as int64 (the same
    bits; None: allocated here).  workspace: uint8, `tensor_range_workspace_numel` elements (None: allocated here).  No host sync."""
    require_cuda(x, out, workspace)
    if x.dtype not in RANGE_DTYPES:
        raise nv.SevaNativeError(f"tensor_range: dtype {x.dtype} (float32, float16, or uint8 holding e4m3 bytes)")
    if x.dim() == 1:
        x = x.unsqueeze(0)
    if x.dim() != 2 or (x.stride(1) != 1 and x.shape[1] != 1):
        raise nv.SevaNativeError(f"tensor_range: a 2-D view with unit inner stride (got shape {tuple(x.shape)}, strides {x.stride()})")
    rows = x.shape[0] if rows is None else int(rows)
    cols = x.shape[1] if cols is None else int(cols)
    if not (0 < rows <= x.shape[0] and 0 < cols <= x.shape[1]):
        raise nv.SevaNativeError(f"tensor_range: rows x cols = {rows} x {cols} outside the view {tuple(x.shape)}")
    pitch = x.stride(0) if rows > 1 else cols
    if pitch < cols:
        raise nv.SevaNativeError(f"tensor_range: row pitch {pitch} below cols {cols} (overlapping rows)")
    if out is None:
        out = torch.empty(RANGE_WORDS, dtype=torch.int64, device=x.device)
    assert out.dtype == torch.int64 and out.numel() == RANGE_WORDS and out.is_contiguous()
    workspace = _workspace(workspace, tensor_range_workspace_numel(rows, cols), x.device, "tensor_range")
    d = nv.RangeDesc()
    d.x, d.dtype, d.rows, d.cols, d.pitch = x.data_ptr(), RANGE_DTYPES[x.dtype], rows, cols, pitch
    d.workspace, d.workspace_bytes, d.out = workspace.data_ptr(), workspace.numel(), out.data_ptr()
    check(_lib().seva_tensor_range(C.byref(d), stream_ptr(x.device)), "seva_tensor_range")
    return out


@_audited("out_f32", "out_f16", "out_f8")
def gemm(
    a: torch.Tensor,
    w: torch.Tensor,
    *,
    bias: torch.Tensor | None = None,
    row_add: torch.Tensor | None = None,
    rows_per_group: int = 0,
    ld_row_add: int = 0,
    residual: torch.Tensor | None = None,
    out_f32: torch.Tensor | None = None,
    out_f16: torch.Tensor | None = None,
    geglu: bool = False,
    col_scale: float = 1.0,
    col_scale_n: int = 0,
    w_exp: torch.Tensor | None = None,
    out_f8: torch.Tensor | None = None,
    ch_stats: torch.Tensor | None = None,
    splitk_ws: torch.Tensor | None = None,
    alg_k: int = 0,
    split_out: bool = False,
) -> None:
    """out = a @ w.T (+bias +row_add[group] +residual); a:[M,K] f16, w:[N,K] f16 (seva_gemm_f16).
    split_out (seva_gemm_f16_split_out): out_f16 is [M, >= 2 NO] and receives [hi | lo] of the fp32 epilogue value (NO = N, GEGLU:
    N / 2); f16 GEMM mode only -- with fp8 operands, out_f8 or ch_stats the call raises.
    alg_k: accounting only -- the reference-equivalent reduction length when K is padded / split-precision (seva_gemm_desc.alg_K).
    splitk_ws (`splitk_workspace`): only convolutions use it (seva_gemm_desc.splitk_ws); accepted and ignored for plain GEMMs.
    ch_stats (`channel_stats_buffer`): receives per-64-row-block, per-channel sum / sum of squares of out_f32 (GroupNorm
    statistics emitted by the epilogue; `groupnorm(stats1=...)`).
    Output features < col_scale_n are multiplied by col_scale in fp32 (plain epilogue only).
    fp8 mode (seva_gemm_fp8): a, w are uint8 tensors of e4m3 bytes and w_exp [N] uint8 the weights' E8M0 scale bytes;
    out_f8 (GEGLU epilogue only) receives the hidden activations as e4m3."""
    fp8 = w_exp is not None
    require_cuda(a, w)
    if split_out and (fp8 or out_f8 is not None or ch_stats is not None or out_f16 is None):
        raise ValueError("gemm(split_out=True) is the f16 GEMM with an out_f16 (no fp8 operands, out_f8 or ch_stats)")
    assert a.dim() == 2 and w.dim() == 2 and a.dtype == w.dtype == (U8 if fp8 else F16)
    M, K = a.shape
    N = w.shape[0]
    d = _gemm_desc(a, w, (M, N, K), lda=a.stride(0), pitch_dim=0, fp8=fp8, geglu=geglu, col_scale=col_scale, col_scale_n=col_scale_n,
                   bias=bias, row_add=row_add, rows_per_group=rows_per_group, ld_row_add=ld_row_add, residual=residual, out_f32=out_f32,
                   out_f16=out_f16, w_exp=w_exp, out_f8=out_f8, ch_stats=ch_stats, splitk_ws=splitk_ws, alg_k=alg_k)
    if fp8:
        assert w_exp.dtype == U8 and w_exp.numel() == N and (out_f8 is None or out_f8.dtype == U8)
        check(_lib().seva_gemm_fp8(C.byref(d), stream_ptr(a.device)), "seva_gemm_fp8")
    elif split_out:
        assert out_f16.dtype == F16 and out_f16.stride(-1) == 1  # (a pitch below 2 NO is the library's error)
        check(_lib().seva_gemm_f16_split_out(C.byref(d), stream_ptr(w.device)), "seva_gemm_f16_split_out")
    else:
        assert out_f8 is None
        check(_lib().seva_gemm_f16(C.byref(d), stream_ptr(w.device)), "seva_gemm_f16")


def gemm_split_out(a: torch.Tensor, w: torch.Tensor, **kw) -> None:
    """`gemm` whose out_f16 is the split-precision operand [hi | lo] of the next GEMM (seva_gemm_f16_split_out)."""
    gemm(a, w, split_out=True, **kw)


STATS_ROWS = 64  # SEVA_CH_STATS_ROWS: rows per block of the epilogue-emitted GroupNorm statistics (seva_gemm_desc.ch_stats)


def channel_stats_shape(rows: int, channels: int) -> tuple[int, int, int]:
    """Shape of the f32 buffer a GEMM / conv fills through `ch_stats`: [row blocks][sum | sum of squares][channel]."""
    return ((rows + STATS_ROWS - 1) // STATS_ROWS, 2, channels)


# Split-K hand-off workspaces that launches have used (data_ptr -> weak reference).  The consumer workgroup of a split tile
# waits for its producer with a BOUNDED spin (csrc/gemm.hip); a give-up leaves a wrong tile and counts itself in int slot
# SPLITK_ERROR_SLOT of the workspace.  `check_handoffs` makes that loud: it is called where a host sync exists anyway (end of a
# sampler trajectory, `prof_collect`, the GPU tests), never inside the step loop.
SPLITK_FLAGS = 16384       # SEVA_SPLITK_FLAGS: int flags at the head of the workspace
SPLITK_ERROR_SLOT = 16383  # SEVA_SPLITK_ERROR_SLOT: a launch has fewer tiles than this
SPLITK_TILE_M = 128        # SEVA_SPLITK_TILE_M x
SPLITK_TILE_N = 160        # SEVA_SPLITK_TILE_N: the fp32 slot of one output tile
SPLITK_MAX_PIXELS = 128    # SEVA_SPLITK_MAX_PIXELS: output pixels per sample up to which a conv qualifies for the split
_handoff_ws: dict = {}


def _register_handoff_ws(ws: torch.Tensor) -> None:
    if ws.data_ptr() not in _handoff_ws:
        import weakref

        _handoff_ws[ws.data_ptr()] = weakref.ref(ws)


def check_handoffs() -> None:
    """Raise SevaNativeError if any split-K consumer gave up waiting for its producer since the last check (the affected
    outputs are wrong).  On error the flag area is zeroed so that a stale flag cannot corrupt the next launch.  Host-syncs."""
    bad = []
    for key, ref in list(_handoff_ws.items()):
        ws = ref()
        if ws is None or ws.data_ptr() != key:
            _handoff_ws.pop(key, None)
            continue
        if torch.cuda.is_current_stream_capturing():
            return
        n = int(ws[SPLITK_ERROR_SLOT:SPLITK_ERROR_SLOT + 1].view(torch.int32).item())
        if n:
            ws[:SPLITK_FLAGS].zero_()
            bad.append(n)
    if bad:
        raise nv.SevaNativeError(
            f"split-K hand-off: {sum(bad)} consumer workgroup(s) gave up waiting for their producer; the outputs of the "
            "affected launches are wrong (flags re-armed; rerun, or set SEVA_CONV_SPLITK=0)")


def splitk_tiles(rows: int, channels: int) -> int:
    """Upper bound of the output tiles of a split-K launch: SPLITK_TILE_M rows by 128 columns, the narrower of the kernels' two widths."""
    return ((rows + SPLITK_TILE_M - 1) // SPLITK_TILE_M) * ((channels + 127) // 128)


def splitk_workspace_numel(tiles: int) -> int:
    """fp32 elements of a split-K workspace for `tiles` output tiles: the flags, then one SPLITK_TILE_M x SPLITK_TILE_N slot each."""
    return SPLITK_FLAGS + tiles * SPLITK_TILE_M * SPLITK_TILE_N


def splitk_workspace(max_rows: int, max_channels: int, device) -> torch.Tensor:
    """Zeroed workspace for `conv3x3(splitk_ws=...)` (seva_gemm_desc.splitk_ws), at least 512 tile slots."""
    return torch.zeros(splitk_workspace_numel(max(512, splitk_tiles(max_rows, max_channels))), dtype=F32, device=device)


def _stats_ptr(ch_stats, M, N, out_f32):
    if ch_stats is None:
        return None
    assert out_f32 is not None and ch_stats.dtype == F32 and ch_stats.is_contiguous()
    assert ch_stats.numel() >= ((M + STATS_ROWS - 1) // STATS_ROWS) * 2 * N
    return ch_stats.data_ptr()


def _pitch(t, dim: int) -> int:
    return t.stride(dim) if t is not None else 0


def _gemm_desc(a, w, mnk, *, lda, pitch_dim, conv=None, a2=None, fp8=False, geglu=False, col_scale=0.0, col_scale_n=0, bias=None,
               row_add=None, rows_per_group=0, ld_row_add=0, residual=None, out_f32=None, out_f16=None, w_exp=None, out_f8=None,
               ch_stats=None, splitk_ws=None, alg_k=0) -> GemmDesc:
    """seva_gemm_desc of every GEMM / conv entry point.  mnk: (M, N, K), K including the K2 columns of a2; pitch_dim: the dimension of
    residual / out_* whose stride is the row pitch (0: GEMM rows, -2: conv pixels); conv: (n, ih, iw, cin, oh, ow, stride, upsample
    code, pad_br_only), None = plain GEMM.  A split-K workspace is handed on (and registered for `check_handoffs`) outside the fp8 mode."""
    d = GemmDesc()
    d.a, d.w = a.data_ptr(), w.data_ptr()
    d.bias, d.row_add, d.residual = ptr(bias), ptr(row_add), ptr(residual)
    d.out_f32, d.out_f16 = ptr(out_f32), ptr(out_f16)
    d.M, d.N, d.K = mnk
    d.alg_K = alg_k
    d.lda = lda
    d.ldr, d.ldo32, d.ldo16 = _pitch(residual, pitch_dim), _pitch(out_f32, pitch_dim), _pitch(out_f16, pitch_dim)
    d.rows_per_group, d.ld_row_add = rows_per_group, ld_row_add
    d.mode, d.epilogue = 0 if conv is None else 1, 1 if geglu else 0
    d.col_scale, d.col_scale_n = col_scale, col_scale_n
    if conv is not None:
        d.n, d.ih, d.iw, d.cin, d.oh, d.ow, d.stride, d.upsample, d.pad_br_only = conv
    if a2 is not None:
        d.a2, d.lda2, d.K2 = a2.data_ptr(), a2.stride(0), a2.shape[1]
    d.ch_stats = _stats_ptr(ch_stats, mnk[0], mnk[1], out_f32)
    if splitk_ws is not None and not fp8:  # `splitk_workspace`: lets small-image convs run as split-K = 2 (seva_hip.h)
        assert splitk_ws.dtype == F32 and splitk_ws.is_contiguous()
        d.splitk_ws, d.splitk_ws_bytes = splitk_ws.data_ptr(), splitk_ws.numel() * 4
        _register_handoff_ws(splitk_ws)
    if fp8:
        d.w_exp, d.out_f8, d.ldo8 = w_exp.data_ptr(), ptr(out_f8), _pitch(out_f8, pitch_dim)
    return d


FF_FUSED_CHANNELS = (64, 128, 256, 320)


def _ff_desc(a, w1, b1, w2, b2, M, c, residual, out_f32, out_f16, ln_x, ln_gamma, ln_beta, ln_eps, w1_exp=None, w2_exp=None) -> nv.FfDesc:
    """seva_ff_desc of both fused feed-forwards: the A operand is `a`, or with ln_x the LayerNorm prologue's (then d.a stays NULL)."""
    d = nv.FfDesc()
    d.w1, d.b1, d.w2, d.b2 = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()
    d.w1_exp, d.w2_exp = ptr(w1_exp), ptr(w2_exp)
    if ln_x is not None:
        d.ln_x, d.ln_gamma, d.ln_beta, d.ldx, d.ln_eps = ln_x.data_ptr(), ln_gamma.data_ptr(), ln_beta.data_ptr(), ln_x.stride(0), ln_eps
    else:
        d.a, d.lda = ptr(a), a.stride(0)
    d.residual, d.out_f32, d.out_f16 = ptr(residual), ptr(out_f32), ptr(out_f16)
    d.M, d.C = M, c
    d.ldr, d.ldo32, d.ldo16 = _pitch(residual, 0), _pitch(out_f32, 0), _pitch(out_f16, 0)
    return d


@_audited("out_f32", "out_f16")
def ff_fused(a: torch.Tensor | None, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, *,
             residual: torch.Tensor | None = None, out_f32: torch.Tensor | None = None,
             out_f16: torch.Tensor | None = None, ln_x: torch.Tensor | None = None,
             ln_gamma: torch.Tensor | None = None, ln_beta: torch.Tensor | None = None, ln_eps: float = 1e-5) -> None:
    """out = W2 . geglu(W1 . a + b1) + b2 (+ residual) in one kernel (seva_ff_fused_f16); a: [M, C] f16, w1: [8C, C] f16
    (interleaved GEGLU layout), w2: [C, 4C] f16; C in FF_FUSED_CHANNELS.  With ln_x ([M, C] f32) the A operand is
    LayerNorm(ln_x) * ln_gamma + ln_beta, computed in the kernel's prologue (a = None)."""
    src = ln_x if ln_x is not None else a
    require_cuda(src, w1, w2)
    M, c = src.shape
    assert (ln_x is not None and ln_x.dtype == F32 and ln_gamma is not None and ln_beta is not None) or a.dtype == F16
    assert w1.dtype == F16 and w2.dtype == F16 and w1.shape == (8 * c, c) and w2.shape == (c, 4 * c)
    assert w1.is_contiguous() and w2.is_contiguous() and c in FF_FUSED_CHANNELS
    d = _ff_desc(a, w1, b1, w2, b2, M, c, residual, out_f32, out_f16, ln_x, ln_gamma, ln_beta, ln_eps)
    check(_lib().seva_ff_fused_f16(C.byref(d), stream_ptr(src.device)), "seva_ff_fused_f16")


FF8_STEP = 128  # hidden features per stage-2 k-step of the e4m3 fused feed-forward (csrc/ff_fp8.h)


def ff8_feature_of(pos: torch.Tensor) -> torch.Tensor:
    """Byte P of a 128-feature step of the stored W2 row holds hidden feature 64 c + 32 q + 8 g + r of that step, where
    P = 64 q + 16 g + 8 c + r (csrc/ff_fp8.h: ff8_feature_of)."""
    return 64 * ((pos >> 3) & 1) + 32 * (pos >> 6) + 8 * ((pos >> 4) & 3) + (pos & 7)


def pack_ff_fp8(w1: torch.Tensor, w2: torch.Tensor):
    """Weights of `ff_fused_fp8` from the fp32 / f16 ones: w1 [8C, C] in the interleaved GEGLU row order, w2 [C, 4C].
    Returns (w1_8 [8C, KP] uint8 e4m3 with zero columns >= C, w1_exp [8C], w2_8 [C, 4C] uint8 with columns permuted into the
    kernel's hidden-feature order, w2_exp [C]); KP = the multiple of 128 at or above C.  Row scales: quantize_weight_fp8."""
    c = w1.shape[1]
    assert w1.shape == (8 * c, c) and w2.shape == (c, 4 * c) and c in FF_FUSED_CHANNELS
    kp = (c + 127) // 128 * 128
    w1p = torch.cat([w1.float(), w1.new_zeros((8 * c, kp - c), dtype=torch.float32)], 1) if kp != c else w1.float()
    w1_8, w1_exp = quantize_weight_fp8(w1p)
    w2_8, w2_exp = quantize_weight_fp8(w2)
    perm = (torch.arange(4 * c, device=w2.device) // FF8_STEP) * FF8_STEP + ff8_feature_of(torch.arange(4 * c, device=w2.device) % FF8_STEP)
    return w1_8, w1_exp, w2_8[:, perm].contiguous(), w2_exp


@_audited("out_f32", "out_f16")
def ff_fused_fp8(a: torch.Tensor | None, w1: torch.Tensor, w1_exp: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor,
                 w2_exp: torch.Tensor, b2: torch.Tensor, *, residual: torch.Tensor | None = None,
                 out_f32: torch.Tensor | None = None, out_f16: torch.Tensor | None = None, ln_x: torch.Tensor | None = None,
                 ln_gamma: torch.Tensor | None = None, ln_beta: torch.Tensor | None = None, ln_eps: float = 1e-5) -> None:
    """e4m3 sibling of `ff_fused` (seva_ff_fused_fp8): weights from `pack_ff_fp8`; a: [M, >= C] uint8 e4m3 bytes (row pitch a
    multiple of 16), or ln_x ([M, C] f32) for the LayerNorm prologue, whose normalised row is rounded once to e4m3.  The hidden
    activations are rounded once to e4m3; fp32 accumulation.  Allocates nothing (graph-capture safe)."""
    src = ln_x if ln_x is not None else a
    require_cuda(src, w1, w2)
    M = src.shape[0]
    c = w2.shape[0]
    kp = (c + 127) // 128 * 128
    assert (ln_x is not None and ln_x.dtype == F32 and ln_x.shape[1] == c and ln_gamma is not None and ln_beta is not None) or \
        (a is not None and a.dtype == U8 and a.shape[1] >= c and a.stride(1) == 1)
    assert w1.dtype == U8 and w2.dtype == U8 and w1.shape == (8 * c, kp) and w2.shape == (c, 4 * c)
    assert w1_exp.dtype == U8 and w2_exp.dtype == U8 and w1_exp.numel() == 8 * c and w2_exp.numel() == c
    assert w1.is_contiguous() and w2.is_contiguous() and c in FF_FUSED_CHANNELS
    d = _ff_desc(a, w1, b1, w2, b2, M, c, residual, out_f32, out_f16, ln_x, ln_gamma, ln_beta, ln_eps, w1_exp, w2_exp)
    check(_lib().seva_ff_fused_fp8(C.byref(d), stream_ptr(src.device)), "seva_ff_fused_fp8")


@_audited("out_f32", "out_f16", "out_f8")
def conv3x3(
    x: torch.Tensor,
    w: torch.Tensor,
    *,
    stride: int = 1,
    upsample: bool = False,
    bias: torch.Tensor | None = None,
    row_add: torch.Tensor | None = None,
    rows_per_group: int = 0,
    ld_row_add: int = 0,
    residual: torch.Tensor | None = None,
    out_f32: torch.Tensor | None = None,
    out_f16: torch.Tensor | None = None,
    pad_br_only: bool = False,
    w_exp: torch.Tensor | None = None,
    ch_stats: torch.Tensor | None = None,
    splitk_ws: torch.Tensor | None = None,
    a2: torch.Tensor | None = None,
    alg_k: int = 0,
    out_f8: torch.Tensor | None = None,
) -> None:
    """3x3 pad-1 conv as implicit GEMM; x: [n, ih, iw, cin] f16 NHWC, w: [cout, 9*cin] f16.
    a2 ([M, K2] f16, K2 % 64 == 0): a second operand folded into the reduction behind the nine taps, w: [cout, 9*cin + K2]
    (seva_gemm_desc.a2: the ResBlock's 1x1 skip conv inside its second 3x3 conv).
    pad_br_only: zero padding at the bottom / right edge only (diffusers Downsample2D, pad (0,1,0,1)).
    fp8 mode (w_exp given): x and w are uint8 tensors of e4m3 bytes, cin % 128 == 0.  The fused upsample and out_f8 (uint8
    [.., cout] e4m3 bytes, saturating RNE of the fp32 result, alone or beside out_f32; pixel pitch and pointer multiples of 8; not
    together with upsample) run on the window kernel only (stride 1, cout % 128 == 0): where it declines, the call raises instead of falling back.
    The stride-2 pad_br_only conv in fp8 mode (the VAE encoder's fp8 downsample convs) takes the per-tap gather by default; with the conv_win
    knob at 1 or 2 it runs on the window kernel's stride-2 family (cout % 128 == 0, no out_f8), and raises where that declines."""
    require_cuda(x, w)
    fp8 = w_exp is not None
    assert x.dtype == w.dtype == (U8 if fp8 else F16) and x.dim() == 4 and x.is_contiguous()
    n, ih, iw, cin = x.shape
    eh, ew = (2 * ih, 2 * iw) if upsample else (ih, iw)
    ps = 1 if pad_br_only else 2
    oh, ow = (eh + ps - 3) // stride + 1, (ew + ps - 3) // stride + 1
    M, N, K = n * oh * ow, w.shape[0], 9 * cin
    if a2 is not None:
        assert not fp8 and not upsample and a2.dtype == F16 and a2.dim() == 2 and a2.stride(1) == 1 and a2.shape[0] == M
        K += a2.shape[1]
    assert w.shape[1] == K
    if fp8:
        assert w_exp.dtype == U8 and w_exp.numel() == N
        if out_f8 is not None:
            assert out_f8.dtype == U8 and out_f8.stride(-1) == 1 and out_f8.shape[-1] >= N
            assert not upsample, "out_f8 and the fused upsample are not available together"
    else:
        assert out_f8 is None, "out_f8 belongs to the fp8 conv (w_exp)"
    d = _gemm_desc(x, w, (M, N, K), lda=cin, pitch_dim=-2, a2=a2, fp8=fp8, bias=bias, row_add=row_add, rows_per_group=rows_per_group,
                   ld_row_add=ld_row_add, residual=residual, out_f32=out_f32, out_f16=out_f16, w_exp=w_exp, out_f8=out_f8,
                   ch_stats=ch_stats, splitk_ws=splitk_ws, alg_k=alg_k,
                   conv=(n, ih, iw, cin, oh, ow, stride, 1 if upsample else 0, 1 if pad_br_only else 0))
    if fp8:
        check(_lib().seva_gemm_fp8(C.byref(d), stream_ptr(x.device)), "seva_gemm_fp8(conv)")
    else:
        check(_lib().seva_gemm_f16(C.byref(d), stream_ptr(x.device)), "seva_gemm_f16(conv)")


def _up_phases(name: str, code: int, what: str, x, w4, bias, out_f32, ch_stats, alg_k) -> None:
    """The two phase operators: seva_gemm_desc.upsample = `code` (2: 160-column tiles, no statistics; 4: 128-column tiles)."""
    require_cuda(x, w4)
    assert x.dtype == w4.dtype == F16 and x.dim() == 4 and x.is_contiguous() and w4.is_contiguous()
    n, ih, iw, cin = x.shape
    assert w4.dim() == 3 and w4.shape[0] == 4 and w4.shape[2] == 4 * cin, "w4: [4, cout, 4 * cin]"
    if code == 2 and ch_stats is not None:
        raise ValueError(f"{name} emits no GroupNorm statistics (ch_stats must be None)")
    if out_f32 is None:
        raise ValueError(f"{name} needs out_f32")
    oh, ow = 2 * ih, 2 * iw
    d = _gemm_desc(x, w4, (n * oh * ow, w4.shape[1], 4 * cin), lda=cin, pitch_dim=-2, conv=(n, ih, iw, cin, oh, ow, 1, code, 0),
                   bias=bias, out_f32=out_f32, ch_stats=ch_stats, alg_k=alg_k)
    check(_lib().seva_gemm_f16(C.byref(d), stream_ptr(x.device)), what)


@_audited("out_f32")
def conv3x3_up_phases(x: torch.Tensor, w4: torch.Tensor, *, bias: torch.Tensor | None = None, out_f32: torch.Tensor | None = None,
                      ch_stats: torch.Tensor | None = None, alg_k: int = 0) -> None:
    """Nearest-2x upsample + 3x3 pad-1 conv as four 2x2 phase convs on the source image (seva_gemm_desc.upsample = 2): 4/9 of the
    FLOPs of `conv3x3(upsample=True)`.  x: [n, ih, iw, cin] f16 NHWC; w4: [4, cout, 4*cin] f16, phase 2 py + px, K ordered
    (a, b, ci): the 3x3 weights that meet on one source pixel, summed (the engine's `combine_up_phases`); out_f32: [n, 2 ih * 2 iw,
    cout].  bias + out_f32 only, cout % 160 == 0.  The path emits no GroupNorm statistics: `ch_stats` must be None (the keyword
    names what the caller has to leave to the consumer's own statistics pass).  alg_k: reduction length the profiler credits
    (9 * cin: the reference operator).  Raises where the window kernel declines: no other kernel reads this weight layout."""
    _up_phases("conv3x3_up_phases", 2, "seva_gemm_f16(conv, upsample phases)", x, w4, bias, out_f32, ch_stats, alg_k)


@_audited("out_f32")
def conv3x3_up_phases128(x: torch.Tensor, w4: torch.Tensor, *, bias: torch.Tensor | None = None, out_f32: torch.Tensor | None = None,
                         ch_stats: torch.Tensor | None = None, alg_k: int = 0) -> None:
    """`conv3x3_up_phases` on the 128-column tiles (seva_gemm_desc.upsample = 4): the VAE decoders' upsample convs.  Same operands
    (x: [n, ih, iw, cin] f16 NHWC; w4: [4, cout, 4*cin] f16 from `combine_up_phases`; out_f32: [n, 2 ih * 2 iw, cout]), cout % 128 == 0,
    linear or 2-D tiles by one image's dimensions, and GroupNorm statistics: `ch_stats` (`channel_stats_shape(n * 4 ih iw, cout)`) gets
    one block per 64 output pixels of one phase, the blocks of an image adding up to that image; it needs ih * iw % 64 == 0.  Raises
    where the window kernel declines: no other kernel reads this weight layout."""
    _up_phases("conv3x3_up_phases128", 4, "seva_gemm_f16(conv, upsample phases, 128 columns)", x, w4, bias, out_f32, ch_stats, alg_k)


@_audited("out")
def attention(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    out: torch.Tensor,
    *,
    nb0: int,
    nb1: int,
    heads: int,
    lq: int,
    lk: int,
    q_strides: tuple[int, int, int],
    k_strides: tuple[int, int, int],
    o_strides: tuple[int, int, int],
    scale: float = 0.125,
    q_prescaled: bool = False,
    split_ws: torch.Tensor | None = None,
) -> None:
    """softmax(q k^T * scale) v per (batch, head), head dim 64 (seva_attention_f16).
    q_prescaled: q already holds q * scale * log2(e) (gemm(col_scale=...)); `scale` is then ignored.

    q/k/v/out are f16 tensors (any views); strides are (batch-outer, batch-inner, token) in
    elements relative to the tensors' data pointers; head h sits at element offset 64*h."""
    require_cuda(q, k, v, out)
    d = _attn_desc(q, k, v, out, nb0, nb1, heads, lq, lk, q_strides, k_strides, o_strides, split_ws, scale, q_prescaled)
    check(_lib().seva_attention_f16(C.byref(d), stream_ptr(q.device)), "seva_attention_f16")


ATTN_SPLIT_MIN_LK = 6144     # SEVA_ATTN_SPLIT_MIN_LK: key length from which seva_attention_f16 splits the K/V range in two
ATTN_SPLIT_ROW_FLOATS = 66   # SEVA_ATTN_SPLIT_ROW_FLOATS: per split and query row, 64 floats of un-normalised O plus (m, l)


def attention_split_workspace_numel(batch: int, heads: int, lq: int, nsplit: int = 2) -> int:
    """fp32 elements of `attention(split_ws=...)`."""
    return nsplit * batch * heads * lq * ATTN_SPLIT_ROW_FLOATS


PV8_MIN_LQ = 2048  # SEVA_ATTN_LONG_MIN_LQ: query length from which seva_attention_f16 runs attn16_kernel, the launches the fp8 P.V kernel replaces


def _v_fp8_parts(batch: int, heads: int, lk: int) -> tuple[int, int]:
    v8, sc = C.c_int64(), C.c_int64()
    check(_lib().seva_attn_v_fp8_size(batch, heads, lk, C.byref(v8), C.byref(sc)), "seva_attn_v_fp8_size")
    return v8.value, sc.value


def v_fp8_workspace_numel(batch: int, heads: int, lk: int) -> int:
    """uint8 elements of the quantised-V workspace of `quantize_v_fp8` / `attention_pv8` (e4m3 values, then E8M0 scales)."""
    v8, sc = _v_fp8_parts(batch, heads, lk)
    return v8 + sc


def _v_fp8_ptrs(ws: torch.Tensor, batch: int, heads: int, lk: int) -> tuple[int, int]:
    v8, sc = _v_fp8_parts(batch, heads, lk)
    assert ws.dtype == U8 and ws.is_contiguous() and ws.numel() >= v8 + sc, "v_fp8 workspace too small"
    return ws.data_ptr(), ws.data_ptr() + v8


def _attn_desc(q, k, v, out, nb0, nb1, heads, lq, lk, q_strides, k_strides, o_strides, split_ws, scale=0.0, q_prescaled=True) -> AttnDesc:
    """seva_attn_desc of the three attention entry points (the fp8 pair: q pre-scaled, `scale` unused; the quantiser passes V alone)."""
    d = AttnDesc()
    d.q, d.k, d.v, d.out = ptr(q), ptr(k), ptr(v), ptr(out)
    d.q_sb0, d.q_sb1, d.q_sl = q_strides
    d.k_sb0, d.k_sb1, d.k_sl = k_strides
    d.o_sb0, d.o_sb1, d.o_sl = o_strides
    d.nb0, d.nb1, d.heads, d.lq, d.lk, d.scale = nb0, nb1, heads, lq, lk, scale
    d.q_prescaled = 1 if q_prescaled else 0
    if split_ws is not None:  # `attention_split_workspace`: lets long key sequences run K/V-split (seva_attn_desc.split_ws)
        assert split_ws.dtype == F32 and split_ws.is_contiguous()
        d.split_ws, d.split_ws_bytes = split_ws.data_ptr(), split_ws.numel() * 4
    return d


@_audited("ws")
def quantize_v_fp8(v: torch.Tensor, ws: torch.Tensor, *, nb0: int, nb1: int, heads: int, lk: int,
                   k_strides: tuple[int, int, int]) -> None:
    """V (f16, the attention strides) -> the e4m3 + E8M0 workspace `attention_pv8` reads (seva_attn_quant_v_fp8).
    ws: uint8, at least v_fp8_workspace_numel(nb0 * nb1, heads, lk) elements."""
    require_cuda(v, ws)
    v8, sc = _v_fp8_ptrs(ws, nb0 * nb1, heads, lk)
    d = _attn_desc(None, None, v, None, nb0, nb1, heads, lk, lk, (0, 0, 0), k_strides, (0, 0, 0), None)
    check(_lib().seva_attn_quant_v_fp8(C.byref(d), v8, sc, stream_ptr(v.device)), "seva_attn_quant_v_fp8")


@_audited("out")
def attention_pv8(q: torch.Tensor, k: torch.Tensor, ws: torch.Tensor, out: torch.Tensor, *, nb0: int, nb1: int, heads: int,
                  lq: int, lk: int, q_strides: tuple[int, int, int], k_strides: tuple[int, int, int],
                  o_strides: tuple[int, int, int], split_ws: torch.Tensor | None = None) -> None:
    """`attention` (q pre-scaled by scale * log2(e)) with P and V in e4m3 on the block-scaled MFMA (seva_attention_pv8); V comes
    from `ws`, filled by `quantize_v_fp8` with the same nb0 / nb1 / heads / lk.  The fp8 mode's opt-in attention sub-option."""
    require_cuda(q, k, ws, out)
    v8, sc = _v_fp8_ptrs(ws, nb0 * nb1, heads, lk)
    d = _attn_desc(q, k, None, out, nb0, nb1, heads, lq, lk, q_strides, k_strides, o_strides, split_ws)
    check(_lib().seva_attention_pv8(C.byref(d), v8, sc, stream_ptr(q.device)), "seva_attention_pv8")


GN_WORKSPACE_SLABS = 1024  # SEVA_GN_WORKSPACE_SLABS


def groupnorm_workspace(n: int, device) -> torch.Tensor:
    return torch.empty(n * GN_WORKSPACE_SLABS * 32 * 2, dtype=F32, device=device)


@_audited("out_f16", "raw_f16", "out_f8")
def groupnorm(
    x1: torch.Tensor,
    x2: torch.Tensor | None,
    gamma: torch.Tensor,
    beta: torch.Tensor,
    out_f16: torch.Tensor,
    workspace: torch.Tensor,
    *,
    groups: int = 32,
    eps: float = 1e-5,
    silu: bool = False,
    dense: torch.Tensor | None = None,
    dense_w: torch.Tensor | None = None,
    dense_b: torch.Tensor | None = None,
    raw_f16: torch.Tensor | None = None,
    out_f8: torch.Tensor | None = None,
    stats1: torch.Tensor | None = None,
    stats2: torch.Tensor | None = None,
    split_out: bool = False,
    split_raw: bool = False,
) -> None:
    """GroupNorm(+SiLU)(+Pluecker modulation) of cat(x1, x2) -> f16; x: [n, hw, c] f32.
    split_out / split_raw: out_f16 / raw_f16 are [n, hw, 2c] and carry [hi | lo] (seva_groupnorm_desc.split_*).
    raw_f16: optional second output, cat(x1, x2) merely cast to f16 (same pass).
    out_f8: optional e4m3 output (uint8 tensor, same layout); out_f16 may then be None.
    stats1 / stats2: the `ch_stats` buffers the kernels that produced x1 / x2 filled (both or none; hw % 64 == 0): the
    statistics pass over the fp32 tensors is skipped."""
    require_cuda(x1, out_f16 if out_f16 is not None else out_f8)
    n, hw, c1 = x1.shape
    c2 = x2.shape[2] if x2 is not None else 0
    d = GroupNormDesc()
    d.x1, d.x2, d.gamma, d.beta = x1.data_ptr(), ptr(x2), gamma.data_ptr(), beta.data_ptr()
    d.dense, d.dense_w, d.dense_b = ptr(dense), ptr(dense_w), ptr(dense_b)
    d.out_f16, d.workspace = ptr(out_f16), workspace.data_ptr()
    d.out_f8 = ptr(out_f8)
    if out_f8 is not None:  # [n, hw, >= c1 + c2] e4m3 bytes; a wider last dim = channel padding of an fp8 conv (pad bytes untouched)
        assert out_f8.dtype == U8 and out_f8.is_contiguous() and out_f8.shape[:2] == (n, hw) and out_f8.shape[2] >= c1 + c2
        d.ld_out_f8 = out_f8.shape[2]
    d.n, d.hw, d.c1, d.c2, d.groups = n, hw, c1, c2, groups
    d.dense_c = dense.shape[-1] if dense is not None else 0
    d.silu, d.eps = 1 if silu else 0, eps
    d.raw_f16 = ptr(raw_f16)
    if stats1 is not None:
        assert hw % STATS_ROWS == 0 and (x2 is None) == (stats2 is None)
        assert stats1.dtype == F32 and stats1.numel() >= (n * hw // STATS_ROWS) * 2 * c1
        assert stats2 is None or (stats2.dtype == F32 and stats2.numel() >= (n * hw // STATS_ROWS) * 2 * c2)
        d.stats1, d.stats2 = stats1.data_ptr(), ptr(stats2)
    else:
        assert stats2 is None
    assert raw_f16 is None or (raw_f16.dtype == F16 and raw_f16.is_contiguous()
                               and raw_f16.numel() == n * hw * (c1 + c2) * (2 if split_raw else 1))
    assert not split_out or (out_f16 is not None and out_f16.is_contiguous() and out_f16.numel() == 2 * n * hw * (c1 + c2))
    d.split_out_f16, d.split_raw_f16 = int(split_out), int(split_raw)
    assert workspace.numel() >= n * GN_WORKSPACE_SLABS * groups * 2
    check(_lib().seva_groupnorm_f16(C.byref(d), stream_ptr(x1.device)), "seva_groupnorm_f16")


@_audited("out_f16")
def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out_f16: torch.Tensor,
              eps: float = 1e-5) -> None:
    """LayerNorm over the last dim; the output dtype selects the kernel: f16, or uint8 = e4m3 bytes (seva_layernorm_fp8)."""
    require_cuda(x, out_f16)
    c = x.shape[-1]
    rows = x.numel() // c
    if out_f16.dtype == F32:
        assert out_f16.data_ptr() != x.data_ptr()
        check(_lib().seva_layernorm_f32(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                        out_f16.data_ptr(), rows, c, eps, stream_ptr(x.device)),
              "seva_layernorm_f32")
        return
    if out_f16.dtype == U8:  # e4m3: the output may be wider than c (K padded to a multiple of 128; pad bytes stay as they are)
        assert out_f16.dim() == 2 and out_f16.stride(1) == 1 and out_f16.shape[0] == rows
        check(_lib().seva_layernorm_fp8(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                        out_f16.data_ptr(), rows, c, eps, out_f16.stride(0), stream_ptr(x.device)),
              "seva_layernorm_fp8")
        return
    assert out_f16.dtype == F16
    check(_lib().seva_layernorm_f16(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                    out_f16.data_ptr(), rows, c, eps, stream_ptr(x.device)),
          "seva_layernorm_f16")


@_audited("out_f16")
def layernorm_split(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out_f16: torch.Tensor, eps: float = 1e-5) -> None:
    """LayerNorm over the last dim as a split-precision operand (seva_layernorm_f16_split): out_f16 [rows, 2 c] f16 = [hi | lo], hi
    bitwise `layernorm`'s f16 output, lo = f16(y - f32(hi))."""
    require_cuda(x, out_f16)
    c = x.shape[-1]
    rows = x.numel() // c
    assert x.dtype == F32 and x.is_contiguous() and out_f16.dtype == F16 and out_f16.is_contiguous() and out_f16.numel() == 2 * rows * c
    check(_lib().seva_layernorm_f16_split(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out_f16.data_ptr(), rows, c, eps,
                                          stream_ptr(x.device)), "seva_layernorm_f16_split")


def quantize_weight_fp8(w: torch.Tensor):
    """[N, K] weights -> (e4m3 bytes [N, K] uint8, E8M0 scale bytes [N] uint8): row n holds e4m3(w[n] * 2^-e[n]) with the
    power-of-two scale 2^e[n] chosen so that max|row| lands in (224, 448] (the top binade of e4m3); the scale byte is
    127 + e[n], what the block-scaled MFMA takes (seva_gemm_fp8).  Pack-time host utility (torch's own e4m3 cast)."""
    w = w.float()
    amax = w.abs().amax(dim=1).clamp_min(1e-30)
    e = torch.ceil(torch.log2(amax / 448.0)).clamp(-126, 127)
    q = (w * torch.exp2(-e)[:, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).contiguous(), (e + 127).to(torch.uint8).contiguous()


def dequantize_weight_fp8(w8: torch.Tensor, w_exp: torch.Tensor) -> torch.Tensor:
    return w8.view(torch.float8_e4m3fn).float() * torch.exp2(w_exp.float() - 127.0)[:, None]


def to_fp8(x: torch.Tensor) -> torch.Tensor:
    """float tensor -> e4m3 bytes (saturating), uint8 view (host utility for tests / one-off conversions)."""
    return x.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)


@_audited("patches_f16")
def clip_preprocess(x: torch.Tensor, patches_f16: torch.Tensor, mean, std, *, out_size: int = 224, patch: int = 14,
                    antialias: bool = True) -> None:
    """kornia-style resize + CLIP normalisation, emitted as the patch matrix of the patch-embedding GEMM
    (seva_clip_preprocess_f16).  x: [n,3,H,W] f32 in [-1,1]; patches_f16: [n*(out/patch)^2, ld >= 3*patch^2] f16."""
    require_cuda(x, patches_f16)
    assert x.dtype == F32 and x.is_contiguous() and x.dim() == 4 and x.shape[1] == 3 and patches_f16.dtype == F16
    n, _, H, W = x.shape
    g = out_size // patch
    assert patches_f16.shape[0] == n * g * g and patches_f16.stride(1) == 1
    m = (C.c_float * 3)(*[float(v) for v in mean])
    sd = (C.c_float * 3)(*[float(v) for v in std])
    check(_lib().seva_clip_preprocess_f16(x.data_ptr(), patches_f16.data_ptr(), n, H, W, out_size, patch,
                                          patches_f16.stride(0), C.cast(m, C.c_void_p), C.cast(sd, C.c_void_p),
                                          1 if antialias else 0, stream_ptr(x.device)), "seva_clip_preprocess_f16")


@_audited("out")
def attention_small(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, *, batch: int, heads: int,
                    L: int, head_dim: int, q_strides: tuple[int, int], k_strides: tuple[int, int],
                    o_strides: tuple[int, int], scale: float) -> None:
    """softmax(q k^T * scale) v, short sequences, any even head dim <= 128 (seva_attention_small_f16); strides are
    (batch, token) in elements, head h at column h * head_dim."""
    require_cuda(q, k, v, out)
    assert q.dtype == k.dtype == v.dtype == out.dtype == F16
    check(_lib().seva_attention_small_f16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), q_strides[0],
                                          q_strides[1], k_strides[0], k_strides[1], o_strides[0], o_strides[1], batch,
                                          heads, L, head_dim, scale, stream_ptr(q.device)), "seva_attention_small_f16")


@_audited("out_f16")
def softmax_rows(x: torch.Tensor, out_f16: torch.Tensor, cols: int, scale: float) -> None:
    """x: [rows, >=cols] f32 -> out_f16: [rows, cols_pad] f16 = softmax(x[:, :cols]*scale), zero padded."""
    require_cuda(x, out_f16)
    rows = x.shape[0]
    check(_lib().seva_softmax_rows_f16(x.data_ptr(), x.stride(0), out_f16.data_ptr(), out_f16.stride(0),
                                       rows, cols, out_f16.shape[1], scale, stream_ptr(x.device)),
          "seva_softmax_rows_f16")


@_audited("out_f16")
def nchw_to_nhwc_f16(x1: torch.Tensor, x2: torch.Tensor | None, out_f16: torch.Tensor,
                     scale: torch.Tensor | None = None, split: bool = False) -> None:
    """split: channels [C, 2C) of the output receive the low parts f16(v - f32(f16(v))) (seva_nchw_to_nhwc_f16_split)."""
    require_cuda(x1, out_f16)
    n, c1 = x1.shape[:2]
    hw = x1.numel() // (n * c1)
    c2 = x2.shape[1] if x2 is not None else 0
    fn = _lib().seva_nchw_to_nhwc_f16_split if split else _lib().seva_nchw_to_nhwc_f16
    check(fn(x1.data_ptr(), c1, ptr(x2), c2, ptr(scale), out_f16.data_ptr(), n, hw, out_f16.shape[-1],
             stream_ptr(x1.device)), "seva_nchw_to_nhwc_f16")


@_audited("out")
def nhwc_to_nchw_f32(x: torch.Tensor, out: torch.Tensor) -> None:
    """x: [n, hw, ld] f32 (first c channels used) -> out [n, c, h, w] f32."""
    require_cuda(x, out)
    n, c = out.shape[:2]
    hw = out.numel() // (n * c)
    check(_lib().seva_nhwc_to_nchw_f32(x.data_ptr(), x.stride(-2), out.data_ptr(), n, c, hw,
                                       stream_ptr(x.device)), "seva_nhwc_to_nchw_f32")


@_audited("out_f16")
def cast_concat_f16(x1: torch.Tensor, x2: torch.Tensor | None, out_f16: torch.Tensor) -> None:
    require_cuda(x1, out_f16)
    c1 = x1.shape[-1]
    rows = x1.numel() // c1
    c2 = x2.shape[-1] if x2 is not None else 0
    check(_lib().seva_cast_concat_f16(x1.data_ptr(), c1, ptr(x2), c2, out_f16.data_ptr(), rows,
                                      stream_ptr(x1.device)), "seva_cast_concat_f16")


@_audited("out_f16")
def cast_concat_f16_split(x1: torch.Tensor, x2: torch.Tensor | None, out_f16: torch.Tensor) -> None:
    """`cast_concat_f16` as a split-precision operand (seva_cast_concat_f16_split): out_f16 [rows, 2 (c1 + c2)] = [f16(v) | f16(v - f32(f16(v)))]."""
    require_cuda(x1, out_f16)
    c1 = x1.shape[-1]
    rows = x1.numel() // c1
    c2 = x2.shape[-1] if x2 is not None else 0
    assert out_f16.dtype == F16 and out_f16.is_contiguous() and out_f16.numel() == 2 * rows * (c1 + c2)
    check(_lib().seva_cast_concat_f16_split(x1.data_ptr(), c1, ptr(x2), c2, out_f16.data_ptr(), rows,
                                            stream_ptr(x1.device)), "seva_cast_concat_f16_split")


@_audited("out")
def bilinear_to_nhwc(src: torch.Tensor, out: torch.Tensor, oh: int, ow: int) -> None:
    require_cuda(src, out)
    n, c, sh, sw = src.shape
    check(_lib().seva_bilinear_to_nhwc_f32(src.data_ptr(), out.data_ptr(), n, c, sh, sw, oh, ow,
                                           stream_ptr(src.device)), "seva_bilinear_to_nhwc_f32")


@_audited("out_f16")
def timestep_embedding_f16(t: torch.Tensor, freqs: torch.Tensor, out_f16: torch.Tensor) -> None:
    require_cuda(t, out_f16)
    assert t.dtype == torch.int64
    n, dim = out_f16.shape
    check(_lib().seva_timestep_embedding_f16(t.data_ptr(), freqs.data_ptr(), out_f16.data_ptr(),
                                             n, dim, stream_ptr(t.device)),
          "seva_timestep_embedding_f16")


@_audited("out_f16")
def silu_f16(x: torch.Tensor, out_f16: torch.Tensor) -> None:
    require_cuda(x, out_f16)
    check(_lib().seva_silu_f16(x.data_ptr(), out_f16.data_ptr(), x.numel(), stream_ptr(x.device)),
          "seva_silu_f16")


@_audited("out")
def add_f32(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor) -> None:
    require_cuda(a, b, out)
    check(_lib().seva_add_f32(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(),
                              stream_ptr(a.device)), "seva_add_f32")


@_audited("out")
def replace_blend(x: torch.Tensor, replace: torch.Tensor, out: torch.Tensor) -> None:
    require_cuda(x, replace, out)
    n, c = x.shape[:2]
    hw = x.numel() // (n * c)
    check(_lib().seva_replace_blend_f32(x.data_ptr(), replace.data_ptr(), out.data_ptr(), n, c, hw,
                                        stream_ptr(x.device)), "seva_replace_blend_f32")


@_audited("out")
def denoiser_combine(net: torch.Tensor, x: torch.Tensor, c_out: torch.Tensor, c_skip: torch.Tensor,
                     out: torch.Tensor) -> None:
    require_cuda(net, x, out)
    n = x.shape[0]
    check(_lib().seva_denoiser_combine_f32(net.data_ptr(), x.data_ptr(), c_out.data_ptr(),
                                           c_skip.data_ptr(), out.data_ptr(), n, x.numel() // n,
                                           stream_ptr(x.device)), "seva_denoiser_combine_f32")


@_audited("out")
def add_noise(x: torch.Tensor, eps: torch.Tensor, noise_scale: torch.Tensor, out: torch.Tensor) -> None:
    require_cuda(x, eps, out)
    n = x.shape[0]
    check(_lib().seva_add_noise_f32(x.data_ptr(), eps.data_ptr(), noise_scale.data_ptr(),
                                    out.data_ptr(), n, x.numel() // n, stream_ptr(x.device)),
          "seva_add_noise_f32")


@_audited("out")
def cfg_euler(x: torch.Tensor, den2: torch.Tensor, scale: torch.Tensor, sigma_hat: torch.Tensor,
              dt: torch.Tensor, out: torch.Tensor) -> None:
    require_cuda(x, den2, out)
    n = x.shape[0]
    check(_lib().seva_cfg_euler_f32(x.data_ptr(), den2.data_ptr(), scale.data_ptr(),
                                    sigma_hat.data_ptr(), dt.data_ptr(), out.data_ptr(), n,
                                    x.numel() // n, stream_ptr(x.device)), "seva_cfg_euler_f32")


@_audited("out", "den_out")
def cfg_multistep(x: torch.Tensor, den: torch.Tensor, scale: torch.Tensor | None, old_den: torch.Tensor | None,
                  a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, out: torch.Tensor,
                  den_out: torch.Tensor | None = None) -> None:
    """out = a[n]*x + b[n]*D + c[n]*old_den and den_out = D in one pass (seva_cfg_multistep_f32), D = u + scale[n]*(cd - u)
    from `den` = [uncond ; cond] when `scale` is given, D = `den` when it is None.  Rows with c[n] == 0 never read their
    history; `old_den=None` is for calls in which every c[n] is 0 (caller's contract).  `den_out` may be `old_den`, `out` may be `x`."""
    require_cuda(x, den, scale, old_den, a, b, c, out, den_out)
    n = x.shape[0]
    for name, t in (("x", x), ("den", den), ("scale", scale), ("old_den", old_den), ("a", a), ("b", b), ("c", c),
                    ("out", out), ("den_out", den_out)):
        if t is not None and (t.dtype != F32 or not t.is_contiguous()):
            raise nv.SevaNativeError(f"cfg_multistep: {name} must be contiguous float32 (got {t.dtype}, strides {t.stride()})")
    for name, t in (("old_den", old_den), ("out", out), ("den_out", den_out)):
        if t is not None and t.shape != x.shape:
            raise nv.SevaNativeError(f"cfg_multistep: {name} has shape {tuple(t.shape)}, x has {tuple(x.shape)}")
    want = ((2 * n if scale is not None else n),) + tuple(x.shape[1:])
    if tuple(den.shape) != want:
        raise nv.SevaNativeError(f"cfg_multistep: den has shape {tuple(den.shape)}, expected {want}")
    for name, t in (("scale", scale), ("a", a), ("b", b), ("c", c)):
        if t is not None and t.numel() != n:
            raise nv.SevaNativeError(f"cfg_multistep: {name} has {t.numel()} entries for {n} images")
    check(_lib().seva_cfg_multistep_f32(x.data_ptr(), den.data_ptr(), ptr(scale), ptr(old_den), a.data_ptr(),
                                        b.data_ptr(), c.data_ptr(), out.data_ptr(), ptr(den_out), n,
                                        x.numel() // max(n, 1), stream_ptr(x.device)), "seva_cfg_multistep_f32")


@_audited("out")
def cfg_combine(den2: torch.Tensor, scale: torch.Tensor, out: torch.Tensor) -> None:
    require_cuda(den2, scale, out)
    n = out.shape[0]
    check(_lib().seva_cfg_combine_f32(den2.data_ptr(), scale.data_ptr(), out.data_ptr(), n,
                                      out.numel() // n, stream_ptr(out.device)), "seva_cfg_combine_f32")


@_audited("out")
def cfg_rescale(den2: torch.Tensor, scale: torch.Tensor, phi: float, out: torch.Tensor,
                mult_out: torch.Tensor | None = None) -> None:
    """Rescaled guidance (seva_cfg_rescale_f32): out[f] = m[f] * g[f] with g = u + scale[f]*(c - u) exactly as `cfg_combine`
    computes it from `den2` = [uncond ; cond], and m[f] = phi * std(c[f]) / std(g[f]) + (1 - phi) from fp64 sums in a fixed order
    (1 where phi == 0 or std(g[f]) == 0).  `mult_out` (n,) receives m.  `out` may not alias `den2`."""
    require_cuda(den2, scale, out, mult_out)
    n = out.shape[0]
    for name, t in (("den2", den2), ("scale", scale), ("out", out), ("mult_out", mult_out)):
        if t is not None and (t.dtype != F32 or not t.is_contiguous()):
            raise nv.SevaNativeError(f"cfg_rescale: {name} must be contiguous float32 (got {t.dtype}, strides {t.stride()})")
    want = (2 * n,) + tuple(out.shape[1:])
    if tuple(den2.shape) != want:
        raise nv.SevaNativeError(f"cfg_rescale: den2 has shape {tuple(den2.shape)}, expected {want}")
    for name, t in (("scale", scale), ("mult_out", mult_out)):
        if t is not None and t.numel() != n:
            raise nv.SevaNativeError(f"cfg_rescale: {name} has {t.numel()} entries for {n} images")
    check(_lib().seva_cfg_rescale_f32(den2.data_ptr(), scale.data_ptr(), float(phi), out.data_ptr(), ptr(mult_out), n,
                                      out.numel() // max(n, 1), stream_ptr(out.device)), "seva_cfg_rescale_f32")


@_audited("out")
def euler_step(x: torch.Tensor, den: torch.Tensor, sigma_hat: torch.Tensor, dt: torch.Tensor,
               out: torch.Tensor) -> None:
    require_cuda(x, den, out)
    n = x.shape[0]
    check(_lib().seva_euler_step_f32(x.data_ptr(), den.data_ptr(), sigma_hat.data_ptr(),
                                     dt.data_ptr(), out.data_ptr(), n, x.numel() // n,
                                     stream_ptr(x.device)), "seva_euler_step_f32")


@_audited("out")
def to_d(x: torch.Tensor, den: torch.Tensor, sigma: torch.Tensor, out: torch.Tensor) -> None:
    require_cuda(x, den, out)
    n = x.shape[0]
    check(_lib().seva_to_d_f32(x.data_ptr(), den.data_ptr(), sigma.data_ptr(), out.data_ptr(), n,
                               x.numel() // n, stream_ptr(x.device)), "seva_to_d_f32")


@_audited("out")
def scale_rows(x: torch.Tensor, s: torch.Tensor, out: torch.Tensor) -> None:
    require_cuda(x, s, out)
    n = x.shape[0]
    check(_lib().seva_scale_rows_f32(x.data_ptr(), s.data_ptr(), out.data_ptr(), n,
                                     x.numel() // n, stream_ptr(x.device)), "seva_scale_rows_f32")


@_audited("out")
def plucker(kinv: torch.Tensor, pose_inv: torch.Tensor, out: torch.Tensor) -> None:
    """out[v] (6,h,w) = Pluecker map of view v from its inverse intrinsics (3x3, latent-pixel units) and the
    inverse relative pose rows (3x4) (seva_plucker_f32)."""
    require_cuda(kinv, pose_inv, out)
    assert kinv.dtype == F32 and pose_inv.dtype == F32 and out.dtype == F32
    assert kinv.is_contiguous() and pose_inv.is_contiguous() and out.is_contiguous()
    V, six, h, w = out.shape
    assert six == 6 and kinv.shape == (V, 3, 3) and pose_inv.shape == (V, 3, 4)
    check(_lib().seva_plucker_f32(kinv.data_ptr(), pose_inv.data_ptr(), out.data_ptr(), V, h, w,
                                  stream_ptr(out.device)), "seva_plucker_f32")


@_audited("c_concat", "uc_concat")
def cond_concat(plucker_maps: torch.Tensor, mask_u8: torch.Tensor, c_concat: torch.Tensor, uc_concat: torch.Tensor) -> None:
    """c_concat = [mask | plucker], uc_concat = [0 | plucker] (seva_cond_concat_f32)."""
    require_cuda(plucker_maps, mask_u8, c_concat, uc_concat)
    V, six, h, w = plucker_maps.shape
    assert six == 6 and mask_u8.dtype == torch.uint8 and mask_u8.numel() == V
    assert c_concat.shape == (V, 7, h, w) and uc_concat.shape == (V, 7, h, w)
    assert plucker_maps.is_contiguous() and c_concat.is_contiguous() and uc_concat.is_contiguous()
    check(_lib().seva_cond_concat_f32(plucker_maps.data_ptr(), mask_u8.data_ptr(), c_concat.data_ptr(),
                                      uc_concat.data_ptr(), V, h, w, stream_ptr(plucker_maps.device)),
          "seva_cond_concat_f32")


@_audited("out")
def image_area_crop(src: torch.Tensor, out: torch.Tensor, *, rh: int, rw: int, ct: int = 0, cl: int = 0, pad_value: float = 0.0,
                    out_mul: float = 1.0, out_add: float = 0.0, context_rgb: torch.Tensor | None = None) -> None:
    """Source conversion + alpha compositing + F.interpolate(mode="area") to (rh, rw) + the (H, W) window at (ct, cl) of the
    resized image (signed; outside = pad_value) + v * out_mul + out_add, bit for bit the reference's CPU arithmetic
    (seva_image_area_crop_u8 / _f32).  src: uint8 (n,h,w,3|4) or fp32 (n,3,h,w), rows dense; out: fp32 (n,3,H,W), planes
    dense, any image pitch; context_rgb: fp32 (h,w,3) alpha background (RGBA sources), None = white."""
    require_cuda(src, out, context_rgb)
    assert out.dtype == F32 and out.dim() == 4 and out.shape[1] == 3
    n, _, H, W = out.shape
    _dense_planes(out, "output")
    d = ImageDesc()
    if src.dtype == torch.uint8:
        assert src.dim() == 4 and src.shape[0] == n and src.shape[3] in (3, 4)
        h, w, c = src.shape[1:]
        assert src.stride(3) == 1 and src.stride(2) == c, "source pixels must be dense in a row"
        d.src_pitch_n, d.src_pitch_c, d.src_pitch_row = src.stride(0), 0, src.stride(1)
        fn, name = _lib().seva_image_area_crop_u8, "seva_image_area_crop_u8"
    else:
        assert src.dtype == F32 and src.dim() == 4 and src.shape[0] == n and src.shape[1] == 3
        h, w, c = src.shape[2], src.shape[3], 3
        assert src.stride(3) == 1, "source rows must be dense"
        d.src_pitch_n, d.src_pitch_c, d.src_pitch_row = src.stride(0), src.stride(1), src.stride(2)
        fn, name = _lib().seva_image_area_crop_f32, "seva_image_area_crop_f32"
    if context_rgb is not None:
        assert context_rgb.dtype == F32 and context_rgb.shape == (h, w, 3) and context_rgb.is_contiguous()
    d.src, d.context_rgb, d.out = src.data_ptr(), ptr(context_rgb), out.data_ptr()
    d.out_pitch_n = out.stride(0)
    d.n, d.h, d.w, d.src_c = n, h, w, c
    d.rh, d.rw, d.ct, d.cl, d.H, d.W = int(rh), int(rw), int(ct), int(cl), H, W
    d.pad_value, d.out_mul, d.out_add = float(pad_value), float(out_mul), float(out_add)
    check(fn(C.byref(d), stream_ptr(out.device)), name)


def rgb_to_u8(x: torch.Tensor, out: torch.Tensor) -> None:
    """x: fp32 (n,3,H,W), planes dense, any image pitch -> out: uint8 (n,H,W,3) contiguous; (v + 1) / 2 * 255, clamped to
    [0, 255], truncated; NaN -> 0 (seva_rgb_to_u8)."""
    require_cuda(x, out)
    assert x.dtype == F32 and x.dim() == 4 and x.shape[1] == 3 and out.dtype == torch.uint8
    n, _, H, W = x.shape
    _dense_planes(x, "input")
    assert out.shape == (n, H, W, 3) and out.is_contiguous()
    check(_lib().seva_rgb_to_u8(x.data_ptr(), x.stride(0), out.data_ptr(), n, H, W, stream_ptr(x.device)), "seva_rgb_to_u8")


def frame_metrics_workspace_numel(n: int, H: int, W: int) -> int:
    """uint8 elements of `frame_metrics(workspace=...)`: one (fp64, u32) partial per 32 x 32 tile of every image."""
    return _size_query(_lib().seva_frame_metrics_size, n, H, W)


def frame_metrics(a: torch.Tensor, b: torch.Tensor, sse: torch.Tensor, ssim_sum: torch.Tensor | None = None,
                  ssim_map: torch.Tensor | None = None, workspace: torch.Tensor | None = None) -> None:
    """Per-frame squared error and SSIM sums of two batches of frames on their uint8 values (seva_frame_metrics; the contract
    is in include/seva_hip.h).  a, b: both uint8 (n,H,W,3), images dense, any image pitch -- or both fp32 (n,3,H,W) in [-1, 1],
    planes dense, any image pitch (scored through the uint8 rule of `rgb_to_u8`).  sse: int64 (n).  ssim_sum: fp64 (n), the
    sum of the SSIM map over 3 (H-10) (W-10) positions (None: squared error only); ssim_map: optional fp32 (n,3,H-10,W-10).
    workspace: uint8, `frame_metrics_workspace_numel` elements (None: allocated here)."""
    require_cuda(a, b, sse, ssim_sum, ssim_map, workspace)
    assert a.dim() == 4 and a.shape == b.shape and a.dtype == b.dtype and a.dtype in (U8, F32)
    d = MetricsDesc()
    d.kind, n, H, W = _frame_layout(a)
    _frame_layout(b)
    assert sse.dtype == torch.int64 and sse.shape == (n,) and sse.is_contiguous()
    assert ssim_sum is None or (ssim_sum.dtype == torch.float64 and ssim_sum.shape == (n,) and ssim_sum.is_contiguous())
    assert ssim_map is None or (ssim_sum is not None and ssim_map.dtype == F32 and ssim_map.is_contiguous()
                                and ssim_map.shape == (n, 3, H - 10, W - 10))
    workspace = _workspace(workspace, frame_metrics_workspace_numel(n, H, W), a.device, "frame_metrics")
    d.a, d.b, d.sse, d.ssim_sum, d.ssim_map, d.workspace = a.data_ptr(), b.data_ptr(), sse.data_ptr(), ptr(ssim_sum), ptr(ssim_map), \
        workspace.data_ptr()
    d.a_pitch_n, d.b_pitch_n, d.workspace_bytes = a.stride(0), b.stride(0), workspace.numel()
    d.n, d.H, d.W, d.ssim = n, H, W, int(ssim_sum is not None)
    check(_lib().seva_frame_metrics(C.byref(d), stream_ptr(a.device)), "seva_frame_metrics")


# --- LPIPS (VGG-16): the operators around the 13 convs (csrc/lpips.hip; the contract is in include/seva_hip.h) ---------
LPIPS_CPAD = 64  # channels of the prepared first-conv operand


@_audited("out_f16")
def lpips_prepare(x: torch.Tensor, out_f16: torch.Tensor) -> None:
    """x: uint8 (n,H,W,3), images dense, any image pitch -- or fp32 (n,3,H,W) in [-1, 1], planes dense, any image pitch (taken
    through the uint8 rule of `rgb_to_u8`) -> out_f16: (n,H,W,64) contiguous, the scaling layer's output in channels 0..2,
    exact zeros above (seva_lpips_prepare_f16)."""
    require_cuda(x, out_f16)
    assert x.dim() == 4 and x.dtype in (U8, F32)
    kind, n, H, W = _frame_layout(x)
    assert out_f16.dtype == F16 and out_f16.shape == (n, H, W, LPIPS_CPAD) and out_f16.is_contiguous()
    check(_lib().seva_lpips_prepare_f16(x.data_ptr(), x.stride(0), kind, out_f16.data_ptr(), n, H, W,
                                        stream_ptr(x.device)), "seva_lpips_prepare_f16")


@_audited("relu_out", "pool_out")
def lpips_relu_pool(x: torch.Tensor, relu_out: torch.Tensor, pool_out: torch.Tensor | None = None) -> None:
    """x: f16 (n,h,w,c) contiguous, c % 64 == 0 -> relu_out (n,h,w,c) = relu(x) (may be x itself) and, when given, pool_out
    (n,h//2,w//2,c) = its 2 x 2 / stride-2 max-pool, floor; NaN -> NaN in both (seva_lpips_relu_pool_f16)."""
    require_cuda(x, relu_out, pool_out)
    assert x.dtype == F16 and x.dim() == 4 and x.is_contiguous()
    n, h, w, c = x.shape
    assert relu_out.dtype == F16 and relu_out.shape == x.shape and relu_out.is_contiguous()
    assert pool_out is None or (pool_out.dtype == F16 and pool_out.shape == (n, h // 2, w // 2, c) and pool_out.is_contiguous())
    check(_lib().seva_lpips_relu_pool_f16(x.data_ptr(), relu_out.data_ptr(), ptr(pool_out), n, h, w, c, stream_ptr(x.device)),
          "seva_lpips_relu_pool_f16")


def lpips_layer_workspace_numel(n: int, hw: int) -> int:
    """uint8 elements of `lpips_layer(workspace=...)`: one fp64 partial per 256 pixels of every pair."""
    return _size_query(_lib().seva_lpips_layer_size, n, hw)


def lpips_layer(fa: torch.Tensor, fb: torch.Tensor, w: torch.Tensor, out: torch.Tensor, workspace: torch.Tensor | None = None) -> None:
    """fa, fb: f16 (n,hw,C) features of the two frames of each pair, pixels dense, any pair pitch (a multiple of 8), C in 64, 128,
    256, 512; w: fp32 (C) -> out: fp64 (n), the sum over the pixels of sum_c w[c] (fa_c / |fa| - fb_c / |fb|)^2
    (seva_lpips_layer).  workspace: uint8, `lpips_layer_workspace_numel` elements (None: allocated here)."""
    require_cuda(fa, fb, w, out, workspace)
    assert fa.dtype == fb.dtype == F16 and fa.dim() == 3 and fa.shape == fb.shape
    n, hw, c = fa.shape
    for x in (fa, fb):
        assert x.stride(2) == 1 and x.stride(1) == c, "features: (n,hw,C) with dense pixels"
    assert w.dtype == F32 and w.shape == (c,) and w.is_contiguous()
    assert out.dtype == torch.float64 and out.shape == (n,) and out.is_contiguous()
    workspace = _workspace(workspace, lpips_layer_workspace_numel(n, hw), fa.device, "lpips_layer")
    d = LpipsLayerDesc()
    d.fa, d.fb, d.w, d.out, d.workspace = fa.data_ptr(), fb.data_ptr(), w.data_ptr(), out.data_ptr(), workspace.data_ptr()
    d.a_pitch_n, d.b_pitch_n, d.workspace_bytes, d.hw = fa.stride(0), fb.stride(0), workspace.numel(), hw
    d.n, d.C = n, c
    check(_lib().seva_lpips_layer(C.byref(d), stream_ptr(fa.device)), "seva_lpips_layer")


# --- benchmark / debugging knobs (read from SEVA_* once at library load; see include/seva_hip.h) ---------
def set_knob(name: str, value: int) -> None:
    check(_lib().seva_set_knob(name.encode(), int(value)), "seva_set_knob")


def last_plan() -> str:
    """Table-row name (csrc/gemm_plan.h) of the last GEMM / conv launch this thread planned, "" before any (seva_last_plan)."""
    return _lib().seva_last_plan().decode()


def get_knob(name: str) -> int:
    v = C.c_int32()
    check(_lib().seva_get_knob(name.encode(), C.byref(v)), "seva_get_knob")
    return v.value


# --- profiling / graphs ---------------------------------------------------------------------
def prof_enable(on: bool) -> None:
    check(_lib().seva_prof_enable(1 if on else 0))


def prof_collect() -> dict:
    ms = (C.c_double * nv.PROF_CLASSES)()
    n = (C.c_int64 * nv.PROF_CLASSES)()
    work = (C.c_double * nv.PROF_CLASSES)()
    nbytes = (C.c_double * nv.PROF_CLASSES)()
    check(_lib().seva_prof_collect(ms, n, work, nbytes), "seva_prof_collect")
    check_handoffs()  # (prof_collect synchronises anyway)
    return {name: {"ms": ms[i], "launches": n[i], "work": work[i], "bytes": nbytes[i]}
            for i, name in enumerate(nv.PROF_NAMES)}


class Graph:
    """hipGraph captured from PyTorch's current stream through the C-ABI helpers."""

    def __init__(self):
        self._exec = C.c_void_p()

    def capture_begin(self, device=None) -> None:
        check(_lib().seva_graph_begin(stream_ptr(device)), "seva_graph_begin")

    def capture_end(self, device=None) -> None:
        check(_lib().seva_graph_end(stream_ptr(device), C.byref(self._exec)), "seva_graph_end")

    def launch(self, device=None) -> None:
        check(_lib().seva_graph_launch(self._exec, stream_ptr(device)), "seva_graph_launch")

    def __del__(self):
        try:
            if self._exec:
                _lib().seva_graph_destroy(self._exec)
        except Exception:
            pass
