"""One exact case list for every row of the GEMM / conv instantiation tables (csrc/gemm_plan.h: SEVA_GEMM_KERNELS, SEVA_WIN_KERNELS).

Every row is a template instantiation of its own (tile walk, LDS layout, epilogue, tail handling), so every row has cases here, and each
case is the smallest launch that takes its row.  Two renderers live in this module so that they cannot drift apart:

* `descriptor(case)`: the line csrc/gemm_plan_dump.cpp reads (CPU; the conventions of gemm() / conv() in tests/test_gemm_plan_cpu.py).
  tests/test_kernel_coverage_cpu.py plans every case with it, checks that the plan names the case's `row`, that the rows of the list are
  exactly the rows of the tables, and that the cases of a row together meet the structural conditions stated there as data.
* `launch(ops, case, t)`: the `seva.ops` call (GPU) on the tensors `t` that `tensors_needed(case)` names.
  tests/test_kernel_coverage_gpu.py compares each launch with an fp64 reference on integer operands and checks through
  `ops.last_plan()` that the launch ran the row the case names.

A row is reached by the default dispatch where that launch is still small, else through a knob (gemm_bm, gemm_bn, gemm_astat, conv_win).
OUT OF SCOPE: the 27 ablation twins (knobs gemm_dbg / gemm_stagger > 0): they are timing builds whose results are wrong by design.

Case fields: `id`; `kind` (gemm, geglu, split_out, conv, conv_a2, phases, phases128); `prec` (f16 or e4m3); `shape` -- (M, N, K) for the
GEMM kinds (N counts weight rows: GEGLU writes N / 2 features), (n, ih, iw, cin, cout) for the conv kinds, with `stride`, `up` (fused
nearest-2x upsample), `pad_br` (bottom / right padding only) and `k2` (columns of the folded second operand); `ops`, the epilogue
operands that are present; `rpg`, the rows per row_add group; `knobs`; `row`, the table row the launch must take.
"""
import os
import shutil
import subprocess
from dataclasses import dataclass

CXX = shutil.which("g++")

# epilogue operands a case may name in `ops` (splitk_ws: the workspace that lets a small-image conv run split-K; a2: the folded operand)
OPERANDS = ("bias", "row_add", "residual", "out_f32", "out_f16", "out_f8", "ch_stats", "w_exp", "splitk_ws", "a2")
GEMM_KINDS = ("gemm", "geglu", "split_out")
CONV_KINDS = ("conv", "conv_a2", "phases", "phases128")
KNOBS = ("gemm_bm", "gemm_bn", "gemm_astat", "conv_win")


@dataclass(frozen=True)
class Case:
    id: str
    kind: str
    prec: str
    shape: tuple
    ops: frozenset
    row: str
    knobs: tuple = ()  # ((name, value), ...)
    rpg: int = 0       # rows per row_add group (0: no row_add)
    stride: int = 1
    up: bool = False
    pad_br: bool = False
    k2: int = 0
    geglu: bool = False  # the GEGLU epilogue (kind geglu; a split_out case may have it too)


def conv_geometry(c: Case):
    """(oh, ow, M, K) of a conv case as the caller states it (ops.conv3x3 / conv3x3_up_phases / conv3x3_up_phases128)"""
    n, ih, iw, cin, _ = c.shape
    sc = 2 if (c.up or c.kind in ("phases", "phases128")) else 1
    ps = 1 if c.pad_br else 2
    oh, ow = (sc * ih + ps - 3) // c.stride + 1, (sc * iw + ps - 3) // c.stride + 1
    K = 4 * cin if c.kind in ("phases", "phases128") else 9 * cin + c.k2
    return oh, ow, n * oh * ow, K


def problem(c: Case):
    """(M, N, K) of the launch"""
    if c.kind in GEMM_KINDS:
        return c.shape
    return conv_geometry(c)[2], c.shape[4], conv_geometry(c)[3]


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU renderer
# ------------------------------------------------------------------------------------------------------------------------------------

def line(**kw):
    return " ".join(f"{k}={v}" for k, v in kw.items())


def descriptor(c: Case) -> str:
    """the descriptor line of csrc/gemm_plan_dump.cpp for this case"""
    M, N, K = problem(c)
    d = dict(v="split_out" if c.kind == "split_out" else "fp8" if c.prec == "e4m3" else "f16", mode=0 if c.kind in GEMM_KINDS else 1,
             M=M, N=N, K=K)
    if c.geglu:
        d.update(epi=1)
    if c.kind in CONV_KINDS:
        n, ih, iw, cin, _ = c.shape
        oh, ow = conv_geometry(c)[:2]
        d.update(n=n, ih=ih, iw=iw, cin=cin, oh=oh, ow=ow, stride=c.stride, up={"phases": 2, "phases128": 4}.get(c.kind, int(c.up)),
                 pad_br=int(c.pad_br))
    if c.k2:
        d.update(K2=c.k2)
    for o in OPERANDS:
        if o in c.ops:
            d[o] = 1
    if "row_add" in c.ops:
        d.update(rpg=c.rpg)
    d.update(dict(c.knobs))
    return line(**d)


def build_plan_dump(tmp_dir, pkg):
    """g++ build of csrc/gemm_plan_dump.cpp (plain C++: no ROCm include path, no HIP) -> plans(lines) -> list of dicts, one per
    descriptor line; plans.tables() -> the rows of the two instantiation tables"""
    exe = os.path.join(str(tmp_dir), "gemm_plan_dump")
    src = os.path.join(pkg, "csrc", "gemm_plan_dump.cpp")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, src], check=True)

    def parse(out):
        return [dict(t.split("=", 1) for t in ln.split("\t")) for ln in out.splitlines()]

    def plans(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        out = parse(r.stdout)
        assert len(out) == len(lines), (len(out), len(lines))
        return out

    def tables():
        return parse(subprocess.run([exe], input="tables\n", capture_output=True, text=True, check=True).stdout)

    plans.tables = tables
    return plans


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU renderer
# ------------------------------------------------------------------------------------------------------------------------------------

def tensors_needed(c: Case):
    """names of the tensors `launch` takes for this case: the operands a / w (conv kinds: x / w) and what `ops` names"""
    return (("a", "w") if c.kind in GEMM_KINDS else ("x", "w")) + tuple(o for o in OPERANDS if o in c.ops)


def launch(ops, c: Case, t: dict) -> None:
    """the `seva.ops` call of this case on the tensors t[name] (device tensors in the layouts of seva/ops.py); the knobs are the caller's
    to set (the `knobs` fixture)"""
    kw = {o: t[o] for o in OPERANDS if o in c.ops}
    if "row_add" in c.ops:
        kw["rows_per_group"] = c.rpg
    if c.kind in GEMM_KINDS:
        ops.gemm(t["a"], t["w"], geglu=c.geglu, split_out=c.kind == "split_out", **kw)
    elif c.kind == "phases":
        ops.conv3x3_up_phases(t["x"], t["w"], **kw)
    elif c.kind == "phases128":
        ops.conv3x3_up_phases128(t["x"], t["w"], **kw)
    else:
        ops.conv3x3(t["x"], t["w"], stride=c.stride, upsample=c.up, pad_br_only=c.pad_br, **kw)


# ------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------------------

_SHORT = {"b": "bias", "ra": "row_add", "res": "residual", "o32": "out_f32", "o16": "out_f16", "o8": "out_f8", "st": "ch_stats",
          "sk": "splitk_ws", "a2": "a2"}
ALL5 = "b ra res o32 o16"
CASES = []


def _add(kind, row, tag, shape, ops, *, e4m3=False, **kw):
    knobs = tuple((k, kw.pop(k)) for k in KNOBS if k in kw)
    names = {_SHORT[o] for o in ops.split()} | ({"w_exp"} if e4m3 else set()) | ({"a2"} if kw.get("k2") else set())
    rpg = kw.pop("rpg", 7) if "row_add" in names else 0  # 7 divides no tile height
    kw.setdefault("geglu", kind == "geglu")
    CASES.append(Case(id=f"{row} | {tag}".replace(" ", "_"), kind=kind, prec="e4m3" if e4m3 else "f16", shape=tuple(shape),
                      ops=frozenset(names), row=row, knobs=knobs, rpg=rpg, **kw))


def _gemm_rows():
    """GEMM mode.  Per row: `tail` = one full tile + a ragged tail, a partial last N-tile, an odd K-tile count, every operand;
    `small` = less than one tile, whole N-tiles, an even K-tile count, the bare output."""
    for e4m3 in (False, True):
        p = " e4m3" if e4m3 else ""
        k3, k4, k6, k7 = (384, 512, 768, 896) if e4m3 else (192, 256, 384, 448)  # 3, 4, 6, 7 K-tiles (64 f16 / 128 e4m3 elements)
        np_ = 208 if e4m3 else 200  # partial against 128 and 160 columns (e4m3: N % 16 == 0)
        kw = dict(e4m3=e4m3)
        for bn, nfull in ((128, 256), (160, 320)):
            wide = dict(gemm_bn=160) if bn == 160 else {}
            # fp32 output (and f16 beside it)
            _add("gemm", f"gemm 64x{bn}{p} f32", "tail", (77, np_, k3), ALL5, **wide, **kw)
            _add("gemm", f"gemm 64x{bn}{p} f32", "small", (37, nfull, k4), "o32", gemm_bm=64, **kw)
            # f16 output only: the ASYNC schedule
            _add("gemm", f"gemm 64x{bn}{p} f16-only", "tail", (77, np_, k3), "b ra o16", **wide, **kw)
            _add("gemm", f"gemm 64x{bn}{p} f16-only", "small", (37, nfull, k4), "o16", gemm_bm=64, **kw)
            if e4m3 and bn == 160:
                continue  # e4m3: 128-row tiles are 128 wide only
            _add("gemm", f"gemm 128x{bn}{p} f32", "tail", (141, np_, k3), ALL5 + " st", **wide, **kw)
            _add("gemm", f"gemm 128x{bn}{p} f32", "small", (37, nfull, k4), "o32", **kw)
            _add("gemm", f"gemm 128x{bn}{p} f16-only", "tail", (141, np_, k7), "b ra o16", gemm_bm=128, **wide, **kw)
            _add("gemm", f"gemm 128x{bn}{p} f16-only", "small", (37, nfull, k6), "o16", **kw)
            if not e4m3:  # K <= 320: the A operand stays in registers
                _add("gemm", f"gemm 128x{bn} f16-only A-in-regs", "tail", (141, np_, 192), "b ra o16", gemm_bm=128, **wide)
                _add("gemm", f"gemm 128x{bn} f16-only A-in-regs", "small", (37, nfull, 256), "o16")
                _add("gemm", f"gemm 128x{bn} f16-only A-in-regs", "k5", (130, nfull, 320), "b o16", gemm_bm=128)
    _add("gemm", "gemm 128x32 f32 narrow", "tail", (141, 20, 192), ALL5)
    _add("gemm", "gemm 128x32 f32 narrow", "small", (37, 32, 256), "o32")
    _add("gemm", "gemm 128x32 f32 narrow", "f16-only", (141, 28, 256), "b o16")
    # 160 x 160: the default from M = 2048 where 128-row tiles would number 320 or more (17 x 19 here: the one launch of the list above
    # 10^9 multiply-adds); below that through gemm_bm (gemm_bn: a partial last tile needs the forced width)
    _add("gemm", "gemm 160x160 f32", "default", (2061, 3040, 192), ALL5)
    _add("gemm", "gemm 160x160 f32", "tail", (173, 200, 192), "b o32", gemm_bm=160, gemm_bn=160)
    _add("gemm", "gemm 160x160 f32", "small", (133, 320, 256), "o32", gemm_bm=160)
    # the split-precision output: one tile shape per width, whatever M and the knobs (N % 160 == 0 <=> 160 columns: no partial tile there)
    _add("split_out", "gemm 128x128 split-out", "tail", (141, 200, 192), ALL5)
    _add("split_out", "gemm 128x128 split-out", "small", (37, 256, 256), "o16")
    _add("split_out", "gemm 128x160 split-out", "tail", (141, 320, 192), ALL5)
    _add("split_out", "gemm 128x160 split-out", "small", (37, 160, 256), "o16")


def _geglu_rows():
    """GEGLU epilogue (bias, out_f32, out_f16, e4m3: out_f8; N = weight rows, N / 2 features; tiles are 128 wide: N = 192 leaves half a tile)"""
    for e4m3 in (False, True):
        p = " e4m3" if e4m3 else ""
        k3, k4, k6, k7 = (384, 512, 768, 896) if e4m3 else (192, 256, 384, 448)
        o8 = " o8" if e4m3 else ""
        kw = dict(e4m3=e4m3)
        _add("geglu", f"geglu 64x128{p}", "tail", (77, 192, k3), "b o32 o16" + o8, **kw)
        _add("geglu", f"geglu 64x128{p}", "small", (37, 256, k4), "o8" if e4m3 else "o16", gemm_bm=64, **kw)
        _add("geglu", f"geglu 128x128{p}", "tail", (141, 192, k7), "b o32 o16" + o8, gemm_bm=128, **kw)
        _add("geglu", f"geglu 128x128{p}", "small", (37, 256, k6), "o8" if e4m3 else "o16", **kw)
        if e4m3:
            _add("geglu", "geglu 64x128 e4m3", "f16", (77, 256, k4), "b o16", **kw)
            _add("geglu", "geglu 128x128 e4m3", "f16", (37, 192, k3), "b o16", **kw)
    _add("geglu", "geglu 128x128 A-in-regs", "tail", (141, 192, 192), "b o16", gemm_bm=128)
    _add("geglu", "geglu 128x128 A-in-regs", "small", (37, 256, 256), "o16")
    _add("geglu", "geglu 160x128", "default", (1037, 192, 448), "b o32 o16")  # K > 320 and M >= 1024
    _add("geglu", "geglu 160x128", "small", (133, 256, 384), "o16", gemm_bm=160)
    _add("geglu", "geglu 64x128", "f32", (77, 256, 256), "o32")
    _add("geglu", "geglu 128x128", "f32", (37, 192, 256), "o32")  # (an fp32 output keeps the A operand staged also for K <= 320)
    _add("geglu", "geglu 160x128", "f32", (133, 192, 448), "o32", gemm_bm=160)
    _add("split_out", "geglu 128x128 split-out", "tail", (141, 192, 192), "b o32 o16", geglu=True)
    _add("split_out", "geglu 128x128 split-out", "small", (37, 256, 256), "o16", geglu=True)


def _gather_rows():
    """The per-tap gather (conv mode of gemm_kernel).  It runs by default where the window kernel does not apply: stride 2, a width that
    is neither a multiple of 128 nor of 160 (nor <= 32), statistics on images of hw % 64 != 0, split-K, the folded second operand."""
    for e4m3 in (False, True):
        p = " e4m3" if e4m3 else ""
        c1, c2 = (128, 256) if e4m3 else (64, 128)  # 9 and 18 K-tiles
        np_ = 208 if e4m3 else 200
        kw = dict(e4m3=e4m3)
        # 64-row tiles: 64 < M, few tiles.  7 x 5 images: a tile straddles two of them
        _add("conv", f"conv gather 64x128{p}", "tail", (2, 7, 5, c1, np_), ALL5, rpg=35, **kw)
        _add("conv", f"conv gather 64x128{p}", "small", (2, 5, 5, c2, 192), "o32", gemm_bm=64, **kw)
        _add("conv", f"conv gather 64x128{p}", "stride2", (3, 10, 9, c1, np_), "b res o16", stride=2, **kw)
        _add("conv", f"conv gather 64x160{p}", "tail", (2, 14, 10, c1, 320), ALL5, stride=2, rpg=35, **kw)
        _add("conv", f"conv gather 64x160{p}", "partial", (2, 7, 5, c1, np_), "b o32", gemm_bn=160, **kw)
        _add("conv", f"conv gather 64x160{p}", "small", (2, 10, 10, c2, 160), "o16", stride=2, gemm_bm=64, **kw)
        # 128-row tiles: statistics (a wave owns a 64-row block), or M <= 64
        _add("conv", f"conv gather 128x128{p}", "tail", (3, 7, 7, c1, np_), ALL5 + " st", rpg=49, **kw)
        _add("conv", f"conv gather 128x128{p}", "small", (2, 5, 5, c2, 192), "o32", **kw)
        _add("conv", f"conv gather 128x128{p}", "stride2-br-odd", (2, 9, 7, c1, np_), "b o32 o16", stride=2, pad_br=True, **kw)
        _add("conv", f"conv gather 128x128{p}", "stride2-br-even", (2, 8, 10, c1, 256), "b o16", stride=2, pad_br=True, **kw)
        _add("conv", f"conv gather 128x128{p}", "stride2-even", (2, 8, 10, c1, np_), "res o32", stride=2, **kw)
    _add("conv", "conv gather 128x32 narrow", "tail", (2, 24, 22, 64, 20), ALL5, stride=2, rpg=132)
    _add("conv", "conv gather 128x32 narrow", "small", (2, 10, 10, 128, 32), "o32", stride=2)
    _add("conv", "conv gather 128x32 narrow", "f16", (2, 10, 10, 128, 32), "b o16", stride=2)
    _add("conv", "conv gather 128x160", "tail", (3, 7, 7, 64, 320), ALL5 + " st", rpg=49)
    _add("conv", "conv gather 128x160", "partial", (3, 7, 7, 64, 200), "b o32", gemm_bm=128, gemm_bn=160)
    _add("conv", "conv gather 128x160", "small", (2, 10, 10, 128, 160), "o16", stride=2)
    _add("conv", "conv gather 160x160", "tail", (2, 11, 9, 64, 320), ALL5, gemm_bm=160, rpg=99)
    _add("conv", "conv gather 160x160", "partial", (2, 11, 9, 64, 200), "b o32", gemm_bm=160, gemm_bn=160)
    _add("conv", "conv gather 160x160", "small", (2, 14, 14, 128, 160), "o16", stride=2, gemm_bm=160)
    # split-K = 2: images of at most 128 pixels, an even K-tile count >= 16 (cin 128: 9 per half, cin 256: 18 per half)
    _add("conv", "conv gather 128x128 split-K", "tail", (3, 7, 7, 128, 200), ALL5 + " st sk", rpg=49)
    _add("conv", "conv gather 128x128 split-K", "small", (2, 5, 5, 256, 256), "o32 sk")
    _add("conv", "conv gather 128x128 split-K", "f16", (2, 5, 5, 256, 256), "b o16 sk")
    _add("conv", "conv gather 128x160 split-K", "tail", (3, 7, 7, 128, 320), ALL5 + " st sk", rpg=49)
    _add("conv", "conv gather 128x160 split-K", "partial", (3, 7, 7, 128, 200), "b o32 sk", gemm_bn=160)
    _add("conv", "conv gather 128x160 split-K", "small", (2, 5, 5, 256, 160), "o16 sk")
    # the fused nearest-2x upsample on the gather (3 x 3 sources: 36 output pixels per image)
    _add("conv", "conv gather upsample 64x128", "tail", (2, 3, 3, 64, 200), ALL5, up=True, rpg=36)
    _add("conv", "conv gather upsample 64x128", "small", (1, 3, 3, 128, 192), "o32", up=True, gemm_bm=64)
    _add("conv", "conv gather upsample 64x128", "f16", (1, 3, 3, 128, 192), "b o16", up=True, gemm_bm=64)
    _add("conv", "conv gather upsample 64x160", "tail", (2, 3, 3, 64, 320), ALL5, up=True, conv_win=0, rpg=36)
    _add("conv", "conv gather upsample 64x160", "partial", (2, 3, 3, 64, 200), "b o32", up=True, gemm_bn=160)
    _add("conv", "conv gather upsample 64x160", "small", (1, 3, 3, 128, 160), "o16", up=True, gemm_bm=64)
    _add("conv", "conv gather upsample 128x32", "tail", (2, 7, 5, 64, 20), ALL5, up=True, rpg=140)
    _add("conv", "conv gather upsample 128x32", "small", (2, 3, 3, 128, 32), "o32", up=True)
    _add("conv", "conv gather upsample 128x32", "f16", (2, 3, 3, 128, 32), "b o16", up=True)
    _add("conv", "conv gather upsample 128x128", "tail", (5, 3, 3, 64, 200), ALL5 + " st", up=True, rpg=36)
    _add("conv", "conv gather upsample 128x128", "small", (1, 3, 3, 128, 192), "o32", up=True)
    _add("conv", "conv gather upsample 128x128", "f16", (1, 3, 3, 128, 192), "b o16", up=True)
    _add("conv", "conv gather upsample 128x160", "tail", (5, 3, 3, 64, 320), ALL5 + " st", up=True, rpg=36)
    _add("conv", "conv gather upsample 128x160", "partial", (5, 3, 3, 64, 200), "b o16", up=True, gemm_bm=128, gemm_bn=160)
    _add("conv", "conv gather upsample 128x160", "small", (1, 3, 3, 128, 160), "o32 st", up=True)
    # the folded second operand: 9 cin / 64 + K2 / 64 K-tiles (cin 64: K2 = 128 -> 11, K2 = 64 -> 10)
    _add("conv_a2", "conv gather + a2 128x128", "tail", (3, 7, 7, 64, 200), ALL5 + " st", k2=128, rpg=49)
    _add("conv_a2", "conv gather + a2 128x128", "small", (2, 5, 5, 64, 192), "o32", k2=64)
    _add("conv_a2", "conv gather + a2 128x160", "tail", (3, 7, 7, 64, 320), ALL5 + " st", k2=128, rpg=49)
    _add("conv_a2", "conv gather + a2 128x160", "partial", (3, 7, 7, 64, 200), "b o32", k2=128, gemm_bn=160)
    _add("conv_a2", "conv gather + a2 128x160", "small", (2, 5, 5, 64, 160), "o32", k2=64)
    _add("conv_a2", "conv gather + a2 160x160", "default", (5, 21, 21, 64, 160), ALL5, k2=64, rpg=441)  # M = 2205 >= 2048
    _add("conv_a2", "conv gather + a2 160x160", "partial", (2, 11, 9, 64, 200), "b o32", k2=128, gemm_bm=160, gemm_bn=160)
    _add("conv_a2", "conv gather + a2 160x160", "small", (2, 7, 7, 64, 160), "o32", k2=128, gemm_bm=160)


def _window_rows():
    """The window-staged conv.  Linear tiles: 9 x 9 / 5 x 5 images (a tile straddles two), 8 x 8 with statistics (hw % 64 == 0).  2-D
    tiles (16 output columns x BM / 16 rows) run where the linear window is too wide: 80-pixel rows, five tile columns."""
    _add("conv", "win 4-wave 160x32 linear narrow", "tail", (2, 9, 9, 64, 20), ALL5, rpg=81)
    _add("conv", "win 4-wave 160x32 linear narrow", "small", (2, 5, 5, 128, 32), "o32")
    _add("conv", "win 4-wave 160x32 linear narrow", "f16", (2, 5, 5, 128, 32), "b o16")
    _add("conv", "win 4-wave 128x32 2-D narrow", "full", (2, 8, 80, 64, 20), ALL5, rpg=640)
    _add("conv", "win 4-wave 128x32 2-D narrow", "bare", (1, 16, 80, 128, 32), "o32")
    _add("conv", "win 4-wave 128x32 2-D narrow", "f16", (1, 8, 80, 64, 32), "b o16")
    _add("conv", "win 4-wave 160x160 linear", "tail", (2, 9, 9, 64, 320), ALL5, rpg=81)
    _add("conv", "win 4-wave 160x160 linear", "small", (2, 5, 5, 128, 160), "o32")
    _add("conv", "win 4-wave 160x160 linear", "f16", (2, 5, 5, 128, 160), "b o16")
    _add("conv", "win 4-wave 128x160 linear stats", "tail", (3, 8, 8, 64, 320), ALL5 + " st")
    _add("conv", "win 4-wave 128x160 linear stats", "small", (1, 8, 8, 128, 160), "o32 st")
    _add("conv", "win 8-wave 256x160 linear stats", "tail", (4, 9, 9, 64, 320), ALL5, conv_win=2, rpg=81)
    _add("conv", "win 8-wave 256x160 linear stats", "stats", (5, 8, 8, 128, 160), "b o32 st", conv_win=2)
    _add("conv", "win 8-wave 256x160 linear stats", "small", (2, 5, 5, 128, 160), "o16", conv_win=2)
    for p, e4m3 in (("", False), (" e4m3", True)):
        c1, c2 = (128, 256) if e4m3 else (64, 128)
        kw = dict(e4m3=e4m3)
        for wv, bm, knob in (("4-wave 128", 128, {}), ("8-wave 256", 256, dict(conv_win=2))):
            th, nt = bm // 16, 4 if bm == 256 else 2
            row = f"win{p} {wv}x128"
            # plain
            _add("conv", f"{row} linear stats", "tail", (nt, 9, 9, c1, 256), ALL5, rpg=81, **knob, **kw)
            _add("conv", f"{row} linear stats", "stats", (nt + 1, 8, 8, c2, 128), "b o32 st", **knob, **kw)
            _add("conv", f"{row} linear stats", "small", (2, 5, 5, c2, 128), "o16", **knob, **kw)
            _add("conv", f"{row} 2-D stats", "full", (2, th, 80, c1, 256), ALL5 + " st", rpg=th * 80, **knob, **kw)
            _add("conv", f"{row} 2-D stats", "bare", (1, 2 * th, 80, c2, 128), "o32", **knob, **kw)
            _add("conv", f"{row} 2-D stats", "f16", (1, th, 80, c1, 128), "b o16", **knob, **kw)
            # fused nearest-2x upsample: the window is staged from the source image; the linear window of a tile holds up to five
            # source rows, too many from 72-pixel (4 waves: 9 tile columns) / 104-pixel (8 waves: 13 tile columns) source rows
            wu = 72 if bm == 128 else 104
            _add("conv", f"{row} linear upsample", "tail", (2 * nt + 1, 3, 3, c1, 256), ALL5, up=True, rpg=36, **knob, **kw)
            _add("conv", f"{row} linear upsample", "stats", (nt + 1, 4, 4, c2, 128), "b o32 st", up=True, **knob, **kw)
            _add("conv", f"{row} linear upsample", "small", (2, 3, 3, c2, 128), "o16", up=True, **knob, **kw)
            _add("conv", f"{row} 2-D upsample", "full", (2, th // 2, wu, c1, 128 if e4m3 and bm == 256 else 256), ALL5 + " st", up=True, rpg=th * wu * 2, **knob, **kw)
            _add("conv", f"{row} 2-D upsample", "bare", (1, th, wu, c2, 128), "o32", up=True, **knob, **kw)
            _add("conv", f"{row} 2-D upsample", "f16", (1, th // 2, wu, c1, 256), "b o16", up=True, **knob, **kw)
            if e4m3:  # the e4m3 output epilogue
                _add("conv", f"{row} linear out_f8", "tail", (nt, 9, 9, c1, 256), ALL5 + " o8", rpg=81, **knob, **kw)
                _add("conv", f"{row} linear out_f8", "stats", (nt + 1, 8, 8, c2, 128), "b o8 o32 st", **knob, **kw)
                _add("conv", f"{row} linear out_f8", "small", (2, 5, 5, c2, 128), "o8", **knob, **kw)
                _add("conv", f"{row} 2-D out_f8", "full", (2, th, 80, c1, 256), ALL5 + " st o8", rpg=th * 80, **knob, **kw)
                _add("conv", f"{row} 2-D out_f8", "bare", (1, 2 * th, 80, c2, 128), "o8", **knob, **kw)
    _add("conv", "win 4-wave 128x160 linear upsample", "tail", (5, 3, 3, 64, 320), ALL5, up=True, rpg=36)
    _add("conv", "win 4-wave 128x160 linear upsample", "stats", (3, 4, 4, 128, 160), "b o32 st", up=True)
    _add("conv", "win 4-wave 128x160 linear upsample", "small", (2, 3, 3, 128, 160), "o16", up=True)
    _add("conv", "win 8-wave 256x160 linear upsample", "tail", (9, 3, 3, 64, 320), ALL5, up=True, conv_win=2, rpg=36)
    _add("conv", "win 8-wave 256x160 linear upsample", "stats", (5, 4, 4, 128, 160), "b o32 st", up=True, conv_win=2)
    _add("conv", "win 8-wave 256x160 linear upsample", "small", (2, 3, 3, 128, 160), "o16", up=True, conv_win=2)
    # e4m3 stride 2 with bottom / right padding: only when the conv_win knob asks for it
    s2 = dict(e4m3=True, stride=2, pad_br=True, conv_win=1)
    _add("conv", "win e4m3 4-wave 128x128 linear stride 2", "odd", (4, 15, 13, 128, 256), ALL5, rpg=42, **s2)
    _add("conv", "win e4m3 4-wave 128x128 linear stride 2", "even-stats", (3, 16, 16, 256, 128), "b o32 st", **s2)
    _add("conv", "win e4m3 4-wave 128x128 linear stride 2", "small", (2, 10, 10, 256, 128), "o16", **s2)
    _add("conv", "win e4m3 4-wave 128x128 2-D stride 2", "odd", (2, 17, 161, 128, 256), ALL5 + " st", rpg=640, **s2)
    _add("conv", "win e4m3 4-wave 128x128 2-D stride 2", "even", (1, 32, 160, 256, 128), "o32", **s2)
    _add("conv", "win e4m3 4-wave 128x128 2-D stride 2", "f16", (1, 16, 160, 128, 128), "b o16", **s2)


def _phase_rows():
    """The nearest-2x upsample + 3x3 conv as four 2x2 phase convs on the source image (bias + out_f32; the 128-column family: + ch_stats).
    The launch's rows are SOURCE pixels; K = 4 cin, always an even K-tile count: the cases vary the parity of the 64-channel slabs."""
    _add("phases", "win phases 4-wave 160x160 linear", "tail", (2, 9, 9, 64, 320), "b o32")
    _add("phases", "win phases 4-wave 160x160 linear", "small", (2, 5, 5, 128, 160), "o32")
    _add("phases", "win phases 8-wave 256x160 linear", "tail", (4, 9, 9, 64, 320), "b o32", conv_win=2)
    _add("phases", "win phases 8-wave 256x160 linear", "small", (2, 5, 5, 128, 160), "o32", conv_win=2)
    for wv, bm, knob in (("4-wave 128", 128, {}), ("8-wave 256", 256, dict(conv_win=2))):
        th, nt = bm // 16, 4 if bm == 256 else 2
        row = f"win phases {wv}x128"
        _add("phases128", f"{row} linear stats", "tail", (nt, 9, 9, 64, 256), "b o32", **knob)
        _add("phases128", f"{row} linear stats", "stats", (nt + 1, 8, 8, 128, 128), "b o32 st", **knob)
        _add("phases128", f"{row} linear stats", "small", (2, 5, 5, 128, 128), "o32", **knob)
        _add("phases128", f"{row} 2-D stats", "full", (2, th, 80, 64, 256), "b o32 st", **knob)
        _add("phases128", f"{row} 2-D stats", "bare", (1, 2 * th, 80, 128, 128), "o32", **knob)


_gemm_rows()
_geglu_rows()
_gather_rows()
_window_rows()
_phase_rows()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), "a case id is used twice"
