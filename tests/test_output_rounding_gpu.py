"""The ONE rounding of every f16 / e4m3 tensor a kernel writes: round to nearest even of the fp32 epilogue
value, subnormals kept, inf on f16 overflow, +-448 on e4m3 overflow, NaN stays NaN.

A. Edge values pushed through every epilogue: each kernel is set up to compute exactly `0 + V` in fp32 in front of its conversion,
   V = rounding ties (both parities of the last mantissa bit), ties +- one fp32 ulp, subnormals, the overflow edge, inf and NaN.
   Expected: torch's CPU cast of V, bit for bit (any NaN payload is NaN; +0 = -0 where the epilogue adds to a zero accumulator).
B. Two outputs of one launch agree on random data: out_f16 is bitwise out_f32.half(), [hi | lo] is the split of out_f32.
C. Narrow-only outputs against fp64 on the operands the kernel sees, with four statistics that see a BIASED rounding (a packed
   round-toward-zero convert gives same 0.50, bias -0.50, gain -3.5e-4, ratio 2.00; rel-L2 bounds of 6e-4 .. 2e-3 pass it):
     same  = share of elements bitwise equal to f16(r64)                    bias = mean of (|out| - |r64|) / ulp(r64)
     gain  = <out, r64> / <r64, r64> - 1                                    ratio = rel_l2(out, r64) / rel_l2(f16(r64), r64)
   Shapes are the smallest that reach each instantiation; three have fewer than 9e4 outputs (conv 2x16x16x160: 81 920, GroupNorm
   3x100x96: 28 800, ff_fused C = 64: 19 200): the sampling noise of `bias` (0.29 / sqrt(N) <= 2.1e-3) and of `gain`
   (2.1e-4 / sqrt(N) <= 1.5e-6) stays more than ten times inside the bounds there too.
D. NaN through the e4m3 conversion is part A's NaN entry on every e4m3 producer; the two conversions inside the fused fp8 feed-forward
   (LayerNorm prologue, hidden value) are reached by a NaN row."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from conftest import rel_l2

F16, F32, F64, U8 = torch.float16, torch.float32, torch.float64, torch.uint8
NAN = float("nan")
QK_C = 0.125 * 1.4426950408889634


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from seva import _native
    _native.load()
    return torch.device("cuda:0")


def _rand(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale + shift


# ------------------------------------------------------------------------------------------------------------ the edge vectors
def _up(x):
    return torch.nextafter(x, torch.full_like(x, math.inf))


def _down(x):
    return torch.nextafter(x, torch.full_like(x, -math.inf))


def _f16_edges() -> torch.Tensor:
    """fp32 vector: for >= 512 f16 bit patterns h (random + forced: zero, subnormals, both mantissa parities, the largest finite), both
    signs: h, the midpoint to its successor in magnitude (exact in fp32; a tie), the midpoint +- one fp32 ulp; then the fixed values."""
    g = torch.Generator().manual_seed(20)
    mag = torch.cat([torch.randint(0, 0x7C00, (512,), generator=g),
                     torch.tensor([0, 1, 2, 3, 0x3FE, 0x3FF, 0x400, 0x401, 0x3C00, 0x3C01, 0x7BFE, 0x7BFF])])
    assert ((mag & 1) == 0).sum() > 100 and ((mag & 1) == 1).sum() > 100 and (mag < 0x400).sum() > 8
    val = lambda m: torch.where(m < 0x7C00, m.clamp_max(0x7BFF).to(torch.int16).view(F16).double(), torch.tensor(65536.0, dtype=F64))
    h, mid = val(mag).float(), ((val(mag) + val(mag + 1)) / 2).float()
    assert torch.equal(mid.double() * 2, val(mag) + val(mag + 1))  # the midpoints are exact in fp32
    pos = torch.cat([h, mid, _up(mid), _down(mid)])
    sign = torch.where(torch.rand(pos.shape, generator=g) < 0.5, -1.0, 1.0)
    forced = torch.cat([t[512:] for t in (h, mid, _up(mid), _down(mid))])
    big = torch.tensor(65520.0)
    fixed = torch.tensor([65504.0, -65504.0, float(_down(big)), 65520.0, 1e30, -1e30, math.inf, -math.inf, NAN,
                          2.0 ** -24, 2.0 ** -25, float(_up(torch.tensor(2.0 ** -25))), 2.0 ** -26])
    v = torch.cat([pos * sign, forced, -forced, fixed])
    # the reference cast is what this file trusts: check it on the ties it was built from (nearest EVEN pattern, inf above 65504)
    want = torch.where((mag & 1) == 0, mag, mag + 1).to(torch.int16)
    assert torch.equal(mid.half().view(torch.int16), want) and torch.equal(_up(mid).half().view(torch.int16), (mag + 1).to(torch.int16))
    assert torch.equal(_down(mid).half().view(torch.int16), mag.to(torch.int16))
    assert torch.equal(fixed.half()[[2, 3, 9, 10, 11, 12]], torch.tensor([65504.0, math.inf, 2.0 ** -24, 0.0, 2.0 ** -24, 0.0]).half())
    return v


def _to8(x):
    return x.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(U8)


def _e4m3_edges() -> torch.Tensor:
    """The same over all 254 non-NaN e4m3 byte patterns (the successor of 448 is taken as 480), + the saturation edge, inf and NaN."""
    mag = torch.arange(0, 0x7F)
    dec = torch.arange(0, 0x80, dtype=U8).view(torch.float8_e4m3fn).double()
    dec[0x7F] = 480.0
    h, mid = dec[mag].float(), ((dec[mag] + dec[mag + 1]) / 2).float()
    pos = torch.cat([h, mid, _up(mid), _down(mid)])
    fixed = torch.tensor([448.0, -448.0, 464.0, 1e4, math.inf, -math.inf, NAN])
    v = torch.cat([pos, -pos, fixed])
    want = torch.where((mag & 1) == 0, mag, mag + 1).clamp_max(0x7E).to(U8)
    assert torch.equal(_to8(mid), want) and torch.equal(_to8(_up(mid)), (mag + 1).clamp_max(0x7E).to(U8))
    assert torch.equal(_to8(_down(mid)), mag.to(U8)) and torch.equal(_to8(-mid), want | 0x80)
    assert _to8(fixed).tolist() == [0x7E, 0xFE, 0x7E, 0x7E, 0x7E, 0xFE, 0x7F]
    return v


@pytest.fixture(scope="module")
def V16():
    return _f16_edges()


@pytest.fixture(scope="module")
def V8():
    return _e4m3_edges()


def _tile(v, shape):
    n = math.prod(shape)
    return v.repeat((n + v.numel() - 1) // v.numel())[:n].view(shape).contiguous()


def _chunks(v, c):
    """v as rows of c values (the tail wraps round): one row per launch of a kernel whose injected operand is a [c] vector"""
    n = (v.numel() + c - 1) // c
    return _tile(v, (n, c))


# ------------------------------------------------------------------------------------------------------------ comparisons
def _first_bad(ok, got, want, src):
    i = int((~ok).flatten().nonzero()[0])
    s = "" if src is None else f", fp32 value {src.flatten()[i].item()!r}"
    return f"{int((~ok).sum())} of {ok.numel()} differ; first at {i}: got {got.flatten()[i].item()!r}, want {want.flatten()[i].item()!r}{s}"


def _assert_f16(got, want, what, zero_sign=True, src=None):
    """f16 tensors equal as bits; any NaN is NaN; +0 = -0 only where an epilogue adds to a zero accumulator (zero_sign)"""
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert got.dtype == F16 and want.dtype == F16 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    ok = (got.view(torch.int16) == want.view(torch.int16)) | (got.isnan() & want.isnan())
    if zero_sign:
        ok |= (got == 0) & (want == 0)
    assert bool(ok.all()), f"{what}: {_first_bad(ok, got, want, src)}"


def _assert_f8(got, want, what, src=None):
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert got.dtype == U8 and want.dtype == U8 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    nan = lambda b: (b & 0x7F) == 0x7F
    ok = (got == want) | (nan(got) & nan(want)) | (((got & 0x7F) == 0) & ((want & 0x7F) == 0))
    assert bool(ok.all()), f"{what}: {_first_bad(ok, got, want, src)}"


def _assert_f32(got, want, what):
    got, want = got.detach().cpu(), want.detach().cpu()
    ok = (got == want) | (got.isnan() & want.isnan())
    assert bool(ok.all()), f"{what}: the fp32 values did not arrive: {_first_bad(ok, got, want, None)}"


def _split_lo(v, hi):
    return (v.float() - hi.float()).half()


def _assert_split(hi, lo, v, what, zero_sign=True):
    """[hi | lo] of the fp32 values v: hi = f16(v); lo = f16(v - f32(hi)) where hi is finite; hi + lo non-finite where hi is +-inf"""
    hi, lo, v = hi.detach().cpu(), lo.detach().cpu(), v.detach().cpu().float()
    _assert_f16(hi, v.half(), what + " (hi)", zero_sign, v)
    fin = torch.isfinite(hi)
    _assert_f16(lo[fin], _split_lo(v, hi)[fin], what + " (lo)", True, v[fin])
    inf = torch.isinf(hi)
    assert not bool(torch.isfinite(hi.float() + lo.float())[inf].any()), what + ": hi = +-inf but hi + lo is finite"


def _rows_uniform(out2d):
    """every row of a 2-D device tensor equals row 0 (bits; NaN = NaN; +0 = -0): checked on the device, row 0 goes to the host"""
    f = out2d.view(torch.float8_e4m3fn).float() if out2d.dtype == U8 else out2d.float()
    ok = (f == f[:1]) | (f.isnan() & f[:1].isnan())
    return bool(ok.all())


# ============================================================================================================ A: edge values
GEMM_KNOBS = {"default": {}, "chunks1-astat0": dict(gemm_chunks=1, gemm_astat=0), "chunks1-astat1": dict(gemm_chunks=1, gemm_astat=1),
              "bn128": dict(gemm_bn=128), "bn160": dict(gemm_bn=160)}


@pytest.mark.parametrize("kn", list(GEMM_KNOBS))
@pytest.mark.parametrize("K", [320, 1280])
def test_a_gemm_epilogues(dev, V16, K, kn, knobs):
    """ops.gemm / ops.gemm_split_out with A = 0 and random W (accumulator +0): residual = V, then bias = every N-wide chunk of V
    (the first is V[0]) without a residual; out_f16 alone, beside out_f32, and through the column scale 1.0."""
    from seva import ops
    knobs(**GEMM_KNOBS[kn])
    M, N = 300, 320
    a = torch.zeros((M, K), dtype=F16, device=dev)
    w = (_rand((N, K), 1) * K ** -0.5).half().to(dev)
    v = _tile(V16, (M, N))
    vd, want = v.to(dev), v.half()
    for both in (False, True):
        o16 = torch.full((M, N), NAN, dtype=F16, device=dev)
        o32 = torch.full((M, N), 7.0, device=dev) if both else None
        ops.gemm(a, w, residual=vd, out_f16=o16, out_f32=o32)
        _assert_f16(o16, want, f"gemm residual = V, out_f32 {both}", src=v)
        if both:
            _assert_f32(o32, v, "gemm residual = V")
    sp = torch.full((M, 2 * N), NAN, dtype=F16, device=dev)
    o32 = torch.full((M, N), 7.0, device=dev)
    ops.gemm_split_out(a, w, residual=vd, out_f16=sp, out_f32=o32)
    _assert_f32(o32, v, "gemm_split_out residual = V")
    _assert_split(sp[:, :N], sp[:, N:], v, "gemm_split_out residual = V")
    for row in _chunks(V16, N):
        wantb = row.half()[None].expand(M, N)
        for kw in (dict(), dict(out_f32=True), dict(col_scale=1.0, col_scale_n=N), dict(out_f32=True, col_scale=1.0, col_scale_n=N)):
            o16 = torch.full((M, N), NAN, dtype=F16, device=dev)
            o32 = torch.full((M, N), 7.0, device=dev) if kw.pop("out_f32", False) else None
            ops.gemm(a, w, bias=row.to(dev), out_f16=o16, out_f32=o32, **kw)
            assert _rows_uniform(o16)
            _assert_f16(o16[:1], wantb[:1], f"gemm bias = V chunk, {kw}, out_f32 {o32 is not None}", src=row)
            if o32 is not None:
                _assert_f32(o32[:1], row[None], "gemm bias = V chunk")
        sp = torch.full((M, 2 * N), NAN, dtype=F16, device=dev)
        ops.gemm_split_out(a, w, bias=row.to(dev), out_f16=sp)
        assert _rows_uniform(sp)
        _assert_split(sp[0, :N], sp[0, N:], row, "gemm_split_out bias = V chunk")


# id: (n, ih, iw, cin, cout, stride, conv_win knob, split-K workspace, K2 of the folded second operand)
CONV_CASES = {
    "2x16x16-64-160-win0": (2, 16, 16, 64, 160, 1, 0, False, 0), "2x16x16-64-160-win1": (2, 16, 16, 64, 160, 1, 1, False, 0),
    "2x16x16-64-160-win2": (2, 16, 16, 64, 160, 1, 2, False, 0), "1x144x144-64-128-2d-tiles": (1, 144, 144, 64, 128, 1, -1, False, 0),
    "2x16x12-64-64-stride2": (2, 16, 12, 64, 64, 2, -1, False, 0), "5x9x9-128-320-splitk": (5, 9, 9, 128, 320, 1, -1, True, 0),
    "3x12x10-64-128-a2": (3, 12, 10, 64, 128, 1, -1, False, 64),
}


def _conv_setup(dev, case, zero_x, knobs):
    """operands of one CONV_CASES entry (x and a2 zero or random); returns (run(**outputs), M, cout, ref() -> fp64 result)"""
    from seva import ops
    from seva._engine import pack_conv3x3
    n, ih, iw, cin, cout, stride, win, splitk, k2 = CONV_CASES[case]
    knobs(conv_win=win)
    oh, ow = (ih - 1) // stride + 1, (iw - 1) // stride + 1
    M = n * oh * ow
    x = torch.zeros((n, ih, iw, cin)) if zero_x else _rand((n, ih, iw, cin), 31)
    wc = _rand((cout, cin, 3, 3), 32, (9 * cin + k2) ** -0.5)
    a2 = (torch.zeros((M, k2)) if zero_x else _rand((M, k2), 33)) if k2 else None
    w2 = _rand((cout, k2), 34, (9 * cin + k2) ** -0.5) if k2 else None
    wp = pack_conv3x3(wc)
    if k2:
        wp = torch.cat([wp, w2.half()], 1).contiguous()
    xh, wp = x.half().to(dev), wp.to(dev)
    kw = {}
    if k2:
        kw["a2"] = a2.half().to(dev)
    if splitk:
        kw["splitk_ws"] = ops.splitk_workspace(M, cout, dev)

    def ref():
        r = F.conv2d(x.half().double().permute(0, 3, 1, 2), wc.half().double(), None, stride=stride, padding=1).permute(0, 2, 3, 1).reshape(M, cout)
        return r + a2.half().double() @ w2.half().double().T if k2 else r

    return (lambda **outs: ops.conv3x3(xh, wp, stride=stride, **kw, **outs)), M, cout, ref


@pytest.mark.parametrize("case", list(CONV_CASES))
def test_a_conv3x3_epilogues(dev, V16, case, knobs):
    """ops.conv3x3 with x = 0 (and a2 = 0), residual = V: the per-tap kernel, both window families, 2-D tiles, stride 2, the split-K
    consumer and the folded second operand; out_f16 alone and beside out_f32."""
    from seva import ops
    from seva._native import SevaNativeError
    run, M, cout, _ = _conv_setup(dev, case, True, knobs)
    v = _tile(V16, (M, cout))
    for both in (False, True):
        o16 = torch.full((M, cout), NAN, dtype=F16, device=dev)
        o32 = torch.full((M, cout), 7.0, device=dev) if both else None
        if CONV_CASES[case][8] and not both:  # the folded second operand exists with an fp32 output only: no f16-only launch to test
            with pytest.raises(SevaNativeError, match="an fp32 output"):
                run(residual=v.to(dev), out_f16=o16)
            continue
        run(residual=v.to(dev), out_f16=o16, out_f32=o32)
        _assert_f16(o16, v.half(), f"conv {case}, out_f32 {both}", src=v)
        if both:
            _assert_f32(o32, v, f"conv {case}")
    ops.check_handoffs()


def _ff_operands(dev, c, M, w2_zero, seed=91):
    from seva._engine import interleave_geglu
    g = torch.Generator().manual_seed(seed + c)
    a = torch.randn(M, c, generator=g).half()
    w1 = (torch.randn(8 * c, c, generator=g) * c ** -0.5).half()
    b1 = 0.3 * torch.randn(8 * c, generator=g)
    w2 = torch.zeros(c, 4 * c).half() if w2_zero else (torch.randn(c, 4 * c, generator=g) * (4 * c) ** -0.5).half()
    b2 = torch.zeros(c) if w2_zero else 0.3 * torch.randn(c, generator=g)
    x = torch.randn(M, c, generator=g) * 2 + 0.3
    gm, bt = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    wi, bi = interleave_geglu(w1, b1)
    return dict(a=a, w1=w1, b1=b1, wi=wi, bi=bi, w2=w2, b2=b2, x=x, gm=gm, bt=bt)


@pytest.mark.parametrize("c", [64, 128, 256, 320])
def test_a_ff_fused_epilogues(dev, V16, c):
    """ops.ff_fused and ops.ff_fused_fp8 with W2 = 0, b2 = 0 (finite hidden activations times zero: accumulator 0), residual = V;
    the plain A operand and the LayerNorm prologue; out_f16 alone and beside out_f32."""
    from seva import ops
    M = 300
    p = _ff_operands(dev, c, M, True)
    d = {k: t.to(dev) for k, t in p.items()}
    v = _tile(V16, (M, c))
    vd, want = v.to(dev), v.half()
    ln = dict(ln_x=d["x"], ln_gamma=d["gm"], ln_beta=d["bt"])
    w1_8, w1_exp, w2_8, w2_exp = (t.to(dev) for t in ops.pack_ff_fp8(p["wi"].float(), p["w2"].float()))
    kp = (c + 127) // 128 * 128
    a8 = torch.zeros((M, kp), dtype=U8, device=dev)
    a8[:, :c] = _to8(p["a"]).to(dev)
    runs = {
        "f16, a": lambda **o: ops.ff_fused(d["a"], d["wi"], d["bi"], d["w2"], d["b2"], residual=vd, **o),
        "f16, LayerNorm prologue": lambda **o: ops.ff_fused(None, d["wi"], d["bi"], d["w2"], d["b2"], residual=vd, **ln, **o),
        "fp8, a": lambda **o: ops.ff_fused_fp8(a8, w1_8, w1_exp, d["bi"], w2_8, w2_exp, d["b2"], residual=vd, **o),
        "fp8, LayerNorm prologue": lambda **o: ops.ff_fused_fp8(None, w1_8, w1_exp, d["bi"], w2_8, w2_exp, d["b2"], residual=vd, **ln, **o),
    }
    for name, run in runs.items():
        for both in (False, True):
            o16 = torch.full((M, c), NAN, dtype=F16, device=dev)
            o32 = torch.full((M, c), 7.0, device=dev) if both else None
            run(out_f16=o16, out_f32=o32)
            _assert_f16(o16, want, f"ff_fused C={c} ({name}), out_f32 {both}", src=v)
            if both:
                _assert_f32(o32, v, f"ff_fused C={c} ({name})")


@pytest.mark.parametrize("c", [64, 320])
def test_d_ff_fused_fp8_keeps_a_nan_row(dev, c):
    """The two e4m3 conversions INSIDE ops.ff_fused_fp8 (the LayerNorm prologue's normalised row, the hidden v gelu(g)) keep NaN: one
    NaN in a row of ln_x (its statistics, so the whole normalised row, turn NaN), or one NaN byte in a row of the e4m3 A operand (every
    hidden value of that row turns NaN), gives that output row NaN and leaves every other row finite.  A clamp that turns NaN into -448
    gives a finite row."""
    from seva import ops
    M, row = 300, 133
    p = _ff_operands(dev, c, M, False)
    d = {k: t.to(dev) for k, t in p.items()}
    w1_8, w1_exp, w2_8, w2_exp = (t.to(dev) for t in ops.pack_ff_fp8(p["wi"].float(), p["w2"].float()))
    kp = (c + 127) // 128 * 128
    a8 = torch.zeros((M, kp), dtype=U8, device=dev)
    a8[:, :c] = _to8(p["a"]).to(dev)
    a8[row, 5] = 0x7F
    x = d["x"].clone()
    x[row, 5] = NAN
    for name, kw in (("LayerNorm prologue", dict(a=None, ln_x=x, ln_gamma=d["gm"], ln_beta=d["bt"])), ("e4m3 A operand", dict(a=a8))):
        o32 = torch.full((M, c), 7.0, device=dev)
        ops.ff_fused_fp8(kw.pop("a"), w1_8, w1_exp, d["bi"], w2_8, w2_exp, d["b2"], out_f32=o32, **kw)
        nan_rows = o32.isnan().all(1).cpu()
        assert bool(nan_rows[row]), f"ff_fused_fp8 C={c} ({name}): the NaN row came out finite: {o32[row, :4].tolist()}"
        other = torch.ones(M, dtype=torch.bool)
        other[row] = False
        assert bool(torch.isfinite(o32.cpu()[other]).all()), f"ff_fused_fp8 C={c} ({name}): NaN outside the NaN row"


@pytest.mark.parametrize("rows,c", [(70, 64), (70, 320), (70, 640), (70, 1280), (65536, 64)])
def test_a_layernorm(dev, V16, V8, rows, c):
    """ops.layernorm (f16 and e4m3 outputs) and ops.layernorm_split with gamma = 0, beta = every c-wide chunk of V; 65536 x 64 is the
    4-rows-per-lane instantiation.  The e4m3 output is written into a wider row (pad bytes stay)."""
    from seva import ops
    x = _rand((rows, c), 5, 3.0, 1.0).to(dev)
    zero = torch.zeros(c, device=dev)
    for row in _chunks(V16, c):
        o16 = torch.full((rows, c), NAN, dtype=F16, device=dev)
        sp = torch.full((rows, 2 * c), NAN, dtype=F16, device=dev)
        ops.layernorm(x, zero, row.to(dev), o16)
        ops.layernorm_split(x, zero, row.to(dev), sp)
        assert _rows_uniform(o16) and _rows_uniform(sp)
        _assert_f16(o16[0], row.half(), f"layernorm {rows}x{c}", src=row)
        _assert_split(sp[0, :c], sp[0, c:], row, f"layernorm_split {rows}x{c}")
    for row in _chunks(V8, c):
        o8 = torch.full((rows, c + 16), 0x55, dtype=U8, device=dev)
        ops.layernorm(x, zero, row.to(dev), o8)
        assert _rows_uniform(o8[:, :c].contiguous()) and bool((o8[:, c:] == 0x55).all())
        _assert_f8(o8[0, :c], _to8(row), f"layernorm e4m3 {rows}x{c}", src=row)


@pytest.mark.parametrize("n,hw,c1,c2", [(2, 100, 64, 32), (2, 256, 320, 0)])
def test_a_groupnorm(dev, V16, V8, n, hw, c1, c2):
    """ops.groupnorm with gamma = 0, beta = every C-wide chunk of V, silu off: plain, the 6-component modulation with zero weights
    (y (1 + 0) + 0), split_out, and the e4m3 output at its own and at a padded pixel pitch (with and without the f16 output)."""
    from seva import ops
    C = c1 + c2
    x1 = _rand((n, hw, c1), 1, 2.0, 0.5).to(dev)
    x2 = _rand((n, hw, c2), 2, 1.0, -1.0).to(dev) if c2 else None
    zero = torch.zeros(C, device=dev)
    ws = ops.groupnorm_workspace(n, dev)
    mod = dict(dense=_rand((n, hw, 6), 3).to(dev), dense_w=torch.zeros((2 * C, 6), device=dev), dense_b=torch.zeros(2 * C, device=dev))
    for row in _chunks(V16, C):
        beta = row.to(dev)
        for name, kw in (("plain", {}), ("modulated", mod)):
            o16 = torch.full((n, hw, C), NAN, dtype=F16, device=dev)
            ops.groupnorm(x1, x2, zero, beta, o16, ws, silu=False, **kw)
            assert _rows_uniform(o16.view(n * hw, C))
            _assert_f16(o16[0, 0], row.half(), f"groupnorm {name} C={C}", src=row)
        sp = torch.full((n, hw, 2 * C), NAN, dtype=F16, device=dev)
        ops.groupnorm(x1, x2, zero, beta, sp, ws, silu=False, split_out=True)
        assert _rows_uniform(sp.view(n * hw, 2 * C))
        _assert_split(sp[0, 0, :C], sp[0, 0, C:], row, f"groupnorm split_out C={C}")
    for row in _chunks(V8, C):
        beta = row.to(dev)
        for pad in (0, 32):
            for with16 in (False, True):
                o8 = torch.full((n, hw, C + pad), 0x55, dtype=U8, device=dev)
                o16 = torch.full((n, hw, C), NAN, dtype=F16, device=dev) if with16 else None
                ops.groupnorm(x1, x2, zero, beta, o16, ws, silu=False, out_f8=o8)
                assert _rows_uniform(o8[..., :C].reshape(n * hw, C)) and bool((o8[..., C:] == 0x55).all())
                _assert_f8(o8[0, 0, :C], _to8(row), f"groupnorm out_f8 C={C} pad {pad} out_f16 {with16}", src=row)
                if with16:
                    _assert_f16(o16[0, 0], row.half(), f"groupnorm f16 beside out_f8 C={C}", src=row)


@pytest.mark.parametrize("n,hw,c1,c2", [(2, 100, 64, 32), (2, 256, 320, 0)])
def test_a_groupnorm_raw_outputs(dev, V16, n, hw, c1, c2):
    """raw_f16 / split_raw: x = V itself (finite entries only: one inf or NaN would turn its group's statistics NaN); the raw output
    is bitwise f16(V), zero signs included, lo = f16(V - f32(hi))."""
    from seva import ops
    C = c1 + c2
    v = _tile(V16[torch.isfinite(V16)], (n, hw, C))
    x1 = v[..., :c1].contiguous().to(dev)
    x2 = v[..., c1:].contiguous().to(dev) if c2 else None
    g, b = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    ws = ops.groupnorm_workspace(n, dev)
    out = torch.empty((n, hw, C), dtype=F16, device=dev)
    raw = torch.full((n, hw, C), NAN, dtype=F16, device=dev)
    ops.groupnorm(x1, x2, g, b, out, ws, silu=False, raw_f16=raw)
    _assert_f16(raw, v.half(), f"groupnorm raw_f16 C={C}", zero_sign=False, src=v)
    raw2 = torch.full((n, hw, 2 * C), NAN, dtype=F16, device=dev)
    ops.groupnorm(x1, x2, g, b, out, ws, silu=False, raw_f16=raw2, split_raw=True)
    _assert_split(raw2[..., :C], raw2[..., C:], v, f"groupnorm split_raw C={C}", zero_sign=False)


def test_a_pure_casts(dev, V16):
    """ops.cast_concat_f16(_split) and ops.nchw_to_nhwc_f16 (scale 1; split=True): V in, f16(V) out, zero signs included."""
    from seva import ops
    rows, c1, c2 = 37, 64, 32
    v = _tile(V16, (rows, c1 + c2))
    a, b = v[:, :c1].contiguous().to(dev), v[:, c1:].contiguous().to(dev)
    o = torch.full((rows, c1 + c2), NAN, dtype=F16, device=dev)
    ops.cast_concat_f16(a, b, o)
    _assert_f16(o, v.half(), "cast_concat_f16", zero_sign=False, src=v)
    sp = torch.full((rows, 2 * (c1 + c2)), NAN, dtype=F16, device=dev)
    ops.cast_concat_f16_split(a, b, sp)
    _assert_split(sp[:, :c1 + c2], sp[:, c1 + c2:], v, "cast_concat_f16_split", zero_sign=False)
    n, ca, cb, h, w = 3, 4, 7, 19, 13
    C = ca + cb
    vi = _tile(V16, (n, C, h, w))
    xa, xb = vi[:, :ca].contiguous().to(dev), vi[:, ca:].contiguous().to(dev)
    one = torch.ones(n, device=dev)
    nhwc = vi.permute(0, 2, 3, 1).reshape(n, h * w, C)
    o = torch.full((n, h * w, 16), NAN, dtype=F16, device=dev)
    ops.nchw_to_nhwc_f16(xa, xb, o, scale=one)
    _assert_f16(o[..., :C], nhwc.half(), "nchw_to_nhwc_f16", zero_sign=False, src=nhwc)
    assert bool((o[..., C:] == 0).all())
    o = torch.full((n, h * w, 24), NAN, dtype=F16, device=dev)
    ops.nchw_to_nhwc_f16(xa, xb, o, scale=one, split=True)
    _assert_split(o[..., :C], o[..., C:2 * C], nhwc, "nchw_to_nhwc_f16 split", zero_sign=False)
    assert bool((o[..., 2 * C:] == 0).all())


@pytest.mark.parametrize("win", [-1, 2])
def test_a_fp8_conv_out_f8(dev, V8, win, knobs):
    """seva_gemm_fp8, conv out_f8 epilogue (the window kernel): x = 0, residual = V; alone and beside out_f32."""
    from seva import ops
    knobs(conv_win=win)
    n, ih, iw, cin, cout = 2, 16, 16, 128, 128
    x8 = torch.zeros((n, ih, iw, cin), dtype=U8, device=dev)
    w8, e8 = (t.to(dev) for t in ops.quantize_weight_fp8(_rand((cout, 9 * cin), 41, 0.02)))
    v = _tile(V8, (n, ih * iw, cout))
    for both in (False, True):
        o8 = torch.full((n, ih * iw, cout), 0x55, dtype=U8, device=dev)
        o32 = torch.full((n, ih * iw, cout), 7.0, device=dev) if both else None
        ops.conv3x3(x8, w8, w_exp=e8, residual=v.to(dev), out_f8=o8, out_f32=o32)
        _assert_f8(o8, _to8(v), f"fp8 conv out_f8 (conv_win {win}), out_f32 {both}", src=v)
        if both:
            _assert_f32(o32, v, "fp8 conv residual = V")


def test_a_fp8_geglu_out_f8(dev, V8):
    """seva_gemm_fp8, GEGLU out_f8 epilogue: A = 0, value bias V / 32 and gate bias 32; both erf forms are 1 well below 32, so
    gelu(32) = 32 exactly and the product is V: asserted on the launch's own out_f32 first."""
    from seva import ops
    M, C, K = 300, 320, 640
    assert V8.numel() <= 4 * C
    row = _tile(V8, (4 * C,))
    bi = torch.stack([(row / 32).view(-1, 32), torch.full((4 * C // 32, 32), 32.0)], 1).reshape(8 * C).to(dev)
    a8 = torch.zeros((M, K), dtype=U8, device=dev)
    w8, e8 = (t.to(dev) for t in ops.quantize_weight_fp8(_rand((8 * C, K), 42, K ** -0.5)))
    for both in (True, False):
        o8 = torch.full((M, 4 * C), 0x55, dtype=U8, device=dev)
        o32 = torch.full((M, 4 * C), 7.0, device=dev) if both else None
        ops.gemm(a8, w8, w_exp=e8, bias=bi, out_f8=o8, out_f32=o32, geglu=True)
        if both:
            assert _rows_uniform(o32)
            _assert_f32(o32[0], row, "fp8 GEGLU (V / 32) gelu(32)")
        assert _rows_uniform(o8)
        _assert_f8(o8[0], _to8(row), f"fp8 GEGLU out_f8, out_f32 {both}", src=row)


# ============================================================================================================ B: paired outputs
def _assert_pair(o32, o16, what):
    _assert_f16(o16, o32.cpu().half(), what + ": out_f16 vs out_f32.half()", zero_sign=False, src=o32.cpu())


@pytest.mark.parametrize("K", [320, 1280])
def test_b_gemm_outputs_agree(dev, K):
    """random data: out_f16 is bitwise out_f32.half(); gemm_split_out's hi is bitwise out_f32.half(), lo f16(out_f32 - f32(hi));
    plain epilogue (bias + row_add + residual) and GEGLU."""
    from seva import ops
    from seva._engine import interleave_geglu
    M, N, C, rpg = 300, 320, 320, 7
    a = _rand((M, K), 1).half().to(dev)
    w = (_rand((N, K), 2) * K ** -0.5).half().to(dev)
    bias, res, radd = _rand((N,), 3).to(dev), _rand((M, N), 4).to(dev), _rand(((M + rpg - 1) // rpg, N), 5).to(dev)
    kw = dict(bias=bias, row_add=radd, rows_per_group=rpg, residual=res)
    o32, o16 = torch.full((M, N), NAN, device=dev), torch.full((M, N), NAN, dtype=F16, device=dev)
    ops.gemm(a, w, out_f32=o32, out_f16=o16, **kw)
    assert torch.isfinite(o32).all()
    _assert_pair(o32, o16, f"gemm K={K}")
    s32, sp = torch.full((M, N), NAN, device=dev), torch.full((M, 2 * N), NAN, dtype=F16, device=dev)
    ops.gemm_split_out(a, w, out_f32=s32, out_f16=sp, **kw)
    assert torch.equal(s32, o32)
    _assert_split(sp[:, :N], sp[:, N:], s32, f"gemm_split_out K={K}", zero_sign=False)
    wi, bi = interleave_geglu((_rand((8 * C, K), 6) * K ** -0.5).half(), _rand((8 * C,), 7))
    wi, bi = wi.to(dev), bi.to(dev)
    g32, g16 = torch.full((M, 4 * C), NAN, device=dev), torch.full((M, 4 * C), NAN, dtype=F16, device=dev)
    ops.gemm(a, wi, bias=bi, out_f32=g32, out_f16=g16, geglu=True)
    assert torch.isfinite(g32).all()
    _assert_pair(g32, g16, f"geglu K={K}")
    s32, sp = torch.full((M, 4 * C), NAN, device=dev), torch.full((M, 8 * C), NAN, dtype=F16, device=dev)
    ops.gemm_split_out(a, wi, bias=bi, out_f32=s32, out_f16=sp, geglu=True)
    assert torch.equal(s32, g32)
    _assert_split(sp[:, :4 * C], sp[:, 4 * C:], s32, f"geglu split_out K={K}", zero_sign=False)


@pytest.mark.parametrize("case", list(CONV_CASES))
def test_b_conv3x3_outputs_agree(dev, case, knobs):
    from seva import ops
    run, M, cout, _ = _conv_setup(dev, case, False, knobs)
    bias, res = _rand((cout,), 35).to(dev), _rand((M, cout), 36).to(dev)
    o32, o16 = torch.full((M, cout), NAN, device=dev), torch.full((M, cout), NAN, dtype=F16, device=dev)
    run(bias=bias, residual=res, out_f32=o32, out_f16=o16)
    ops.check_handoffs()
    assert torch.isfinite(o32).all()
    _assert_pair(o32, o16, f"conv {case}")


# ============================================================================================================ C: against fp64
def _half_of_f64(r64):
    return torch.from_numpy(r64.numpy().astype(np.float16))  # (numpy rounds fp64 -> f16 once; torch goes through fp32)


def _rounding_stats(out, r64, what):
    out, r64 = out.detach().cpu().contiguous(), r64.detach().cpu().double().contiguous()
    assert out.dtype == F16 and out.shape == r64.shape and torch.isfinite(out).all(), what
    want = _half_of_f64(r64)
    ulp = torch.exp2(torch.floor(torch.log2(r64.abs().clamp_min(2.0 ** -14))) - 10)
    o = out.double()
    st = dict(n=out.numel(),
              same=float((out.view(torch.int16) == want.view(torch.int16)).double().mean()),
              bias=float(((o.abs() - r64.abs()) / ulp).mean()),
              gain=float((o * r64).sum() / (r64 * r64).sum() - 1.0),
              ratio=rel_l2(o, r64) / rel_l2(want.double(), r64))
    print(f"\n[rounding] {what}: N {st['n']}, same {st['same']:.5f}, bias {st['bias']:+.5f}, gain {st['gain']:+.2e}, ratio {st['ratio']:.4f}")
    return st


def _check(st, what, same=0.99, same_ratio=True):
    """same: 0.99 where the output cast is the only rounding, 0.95 behind an approximated transcendental or a second rounding;
    same_ratio=False (attention: the f16 rounding of P adds noise of the output rounding's own size): bias and gain only."""
    assert abs(st["bias"]) <= 0.05 and abs(st["gain"]) <= 3e-5, (what, st)
    if same_ratio:
        assert st["same"] >= same and st["ratio"] <= 1.05, (what, st)


@pytest.mark.parametrize("rows,c", [(1001, 320), (333, 1280), (4096, 64)])
def test_c_layernorm(dev, rows, c):
    from seva import ops
    x = _rand((rows, c), 1, 3.0, 1.0)
    g, b = 1 + 0.1 * _rand((c,), 2), 0.1 * _rand((c,), 3)
    out = torch.full((rows, c), NAN, dtype=F16, device=dev)
    ops.layernorm(x.to(dev), g.to(dev), b.to(dev), out)
    r64 = F.layer_norm(x.double(), (c,), g.double(), b.double(), 1e-5)
    _check(_rounding_stats(out, r64, f"layernorm {rows}x{c}"), "layernorm")


@pytest.mark.parametrize("silu,dense", [(False, False), (True, False), (True, True)], ids=["plain", "silu", "silu-modulated"])
@pytest.mark.parametrize("n,hw,c1,c2", [(2, 256, 320, 0), (3, 100, 64, 32)])
def test_c_groupnorm(dev, n, hw, c1, c2, silu, dense):
    """test_groupnorm's input distribution.  Plain: the output cast is the only rounding.  With SiLU (exp + rcp approximations,
    outputs near zero) and the modulation: same >= 0.95."""
    from seva import ops
    C = c1 + c2
    x1, x2 = _rand((n, hw, c1), 1, 2.0, 0.5), (_rand((n, hw, c2), 2, 1.0, -1.0) if c2 else None)
    gamma, beta = 1 + 0.1 * _rand((C,), 3), 0.1 * _rand((C,), 4)
    dm, dw, db = _rand((n, hw, 6), 5), _rand((2 * C, 6), 6, 0.3), _rand((2 * C,), 7, 0.1)
    eps = 1e-5 if silu else 1e-6
    out = torch.full((n, hw, C), NAN, dtype=F16, device=dev)
    kw = dict(dense=dm.to(dev), dense_w=dw.to(dev), dense_b=db.to(dev)) if dense else {}
    ops.groupnorm(x1.to(dev), x2.to(dev) if c2 else None, gamma.to(dev), beta.to(dev), out, ops.groupnorm_workspace(n, dev), eps=eps, silu=silu, **kw)
    x = (torch.cat([x1, x2], -1) if c2 else x1).double()
    r64 = F.group_norm(x.transpose(1, 2), 32, gamma.double(), beta.double(), eps).transpose(1, 2)
    if silu:
        r64 = F.silu(r64)
    if dense:
        d = dm.double() @ dw.double().T + db.double()
        r64 = r64 * (1 + d[..., :C]) + d[..., C:]
    what = f"groupnorm {n}x{hw}x{c1}+{c2} silu {silu} modulated {dense}"
    _check(_rounding_stats(out, r64, what), what, same=0.95 if silu else 0.99)


def test_c_silu(dev):
    from seva import ops
    x = _rand((200000,), 1, 3.0)
    out = torch.full((200000,), NAN, dtype=F16, device=dev)
    ops.silu_f16(x.to(dev), out)
    _check(_rounding_stats(out, F.silu(x.double()), "silu_f16"), "silu_f16")


def test_c_softmax_rows(dev):
    """64 x 5183 padded to 5248: exp2 approximation and a reciprocal in front of the cast (same >= 0.95)."""
    from seva import ops
    rows, cols, pad, scale = 64, 5183, 5248, 0.3
    x = _rand((rows, cols), 1, 5.0)
    out = torch.full((rows, pad), NAN, dtype=F16, device=dev)
    ops.softmax_rows(x.to(dev), out, cols, scale)
    assert bool((out[:, cols:] == 0).all())
    _check(_rounding_stats(out[:, :cols], torch.softmax(x.double() * scale, -1), "softmax_rows 64x5183"), "softmax_rows", same=0.95)


@pytest.mark.parametrize("astat", [0, 1])
@pytest.mark.parametrize("K", [320, 1280])
def test_c_gemm_f16_only(dev, K, astat, knobs):
    from seva import ops
    knobs(gemm_chunks=1, gemm_astat=astat)
    M, N = 300, 320
    a, w, bias = _rand((M, K), 1).half(), (_rand((N, K), 2) * K ** -0.5).half(), _rand((N,), 3)
    out = torch.full((M, N), NAN, dtype=F16, device=dev)
    ops.gemm(a.to(dev), w.to(dev), bias=bias.to(dev), out_f16=out)
    r64 = a.double() @ w.double().T + bias.double()
    what = f"gemm {M}x{N}x{K} f16 only, astat {astat}"
    _check(_rounding_stats(out, r64, what), what)


@pytest.mark.parametrize("M,C,K", [(300, 320, 320), (1000, 640, 640)])
def test_c_geglu_f16_only(dev, M, C, K):
    """the erf approximation (8.8e-7 absolute) in front of the cast: same >= 0.95"""
    from seva import ops
    from seva._engine import interleave_geglu
    a, w, b = _rand((M, K), 71).half(), (_rand((8 * C, K), 72) * K ** -0.5).half(), _rand((8 * C,), 73)
    wi, bi = interleave_geglu(w, b)
    out = torch.full((M, 4 * C), NAN, dtype=F16, device=dev)
    ops.gemm(a.to(dev), wi.to(dev), bias=bi.to(dev), out_f16=out, geglu=True)
    y = a.double() @ w.double().T + b.double()
    r64 = y[:, :4 * C] * F.gelu(y[:, 4 * C:])
    what = f"geglu {M}x{C}x{K} f16 only"
    _check(_rounding_stats(out, r64, what), what, same=0.95)


@pytest.mark.parametrize("case", ["2x16x16-64-160-win0", "2x16x16-64-160-win1", "2x16x16-64-160-win2"])
def test_c_conv3x3_f16_only(dev, case, knobs):
    run, M, cout, r64 = _conv_setup(dev, case, False, knobs)
    bias = _rand((cout,), 35)
    out = torch.full((M, cout), NAN, dtype=F16, device=dev)
    run(bias=bias.to(dev), out_f16=out)
    _check(_rounding_stats(out, r64() + bias.double(), f"conv {case} f16 only"), case)


@pytest.mark.parametrize("c", [64, 320])
def test_c_ff_fused(dev, c):
    """The reference rounds the hidden v gelu(g) to f16 ONCE, nearest-even (what the kernel's header states), then multiplies by W2 in
    fp64: `gain` is the check on the hidden rounding too.  same >= 0.95 (erf approximation + second rounding)."""
    from seva import ops
    M = 300
    p = _ff_operands(dev, c, M, False)
    d = {k: t.to(dev) for k, t in p.items()}
    res = _rand((M, c), 8)
    out = torch.full((M, c), NAN, dtype=F16, device=dev)
    ops.ff_fused(d["a"], d["wi"], d["bi"], d["w2"], d["b2"], residual=res.to(dev), out_f16=out)
    y = p["a"].double() @ p["w1"].double().T + p["b1"].double()
    hid = _half_of_f64(y[:, :4 * c] * F.gelu(y[:, 4 * c:])).double()
    r64 = hid @ p["w2"].double().T + p["b2"].double() + res.double()
    _check(_rounding_stats(out, r64, f"ff_fused C={c} M={M}"), f"ff_fused {c}", same=0.95)


def _attn_r64(q, k, v, log2_units):
    """[B, L, H, D] f16 operands as the kernel sees them -> fp64 softmax(q k^T) v, [B, Lq, H, D]"""
    qd, kd, vd = (t.double().transpose(1, 2) for t in (q, k, v))
    s = qd @ kd.transpose(-1, -2) * (math.log(2.0) if log2_units else q.shape[-1] ** -0.5)
    return (torch.softmax(s, -1) @ vd).transpose(1, 2)


ATTN_CASES = {  # B, H, Lq, Lk, attn_two knob
    "attn_kernel-4x64": (4, 2, 200, 200, -1), "attn2": (1, 3, 512, 512, 1), "attn16": (1, 1, 2048, 2048, -1),
}


@pytest.mark.parametrize("case", list(ATTN_CASES))
def test_c_attention(dev, case, knobs):
    """P is packed to f16 with round-to-nearest-even and the row sum is taken from the rounded P.  |bias| <= 0.05 and |gain| <= 3e-5
    are asserted (the f16 parity mode rests on both); same and ratio are printed only (the f16 rounding of P adds noise of the output
    rounding's own size).

    Measured on MI355X (same / bias / gain / ratio), with the round-toward-zero pack these kernels had, and with the nearest-even one:
        attn_kernel<4, 64> (4, 2, 200, 200)      0.5547  +0.0691  +3.19e-5  1.507   ->   0.5964  +0.0007  +2.27e-6  1.359
        attn2_kernel (1, 3, 512, 512)            0.5539  +0.0684  +9.40e-6  1.481   ->   0.5818  +0.0308  +3.38e-6  1.391
        attn16_kernel (1, 1, 2048, 2048)         0.5724  +0.0285  +3.40e-6  1.423   ->   0.5882  +0.0163  +4.41e-7  1.378
        attn_kernel<1, 32>, T = 21 (below)       0.5691  +0.1332  +5.83e-5  1.466   ->   0.6640  +0.0412  +3.24e-7  1.203
        attention_small (2, 16, 257, 80)         0.9977  +0.0002  -2.48e-7  1.000        (fp32 P: unchanged)
    A truncated P cancels in P V / sum(P) to FIRST order only: the key that sets the exponent reference has P = 1.0 exactly and loses
    nothing, every other key loses 2^-11 of its weight on average, so each row leans towards the value of its heaviest key, which is
    also the largest part of the exact result: the output came out too large by ~2^-11 w_max (1 - w_max), more the fewer keys share
    a row.  An emulation on the CPU (P = exp2(s - reference) truncated / rounded to f16, O = P V / sum(P)) reproduces both columns.
    The remaining `bias` is the P noise rectified on outputs near zero (noise not proportional to the element), not a gain."""
    from seva import ops
    B, H, Lq, Lk, two = ATTN_CASES[case]
    knobs(attn_two=two)
    C = 64 * H
    q, k, v = (_rand((B, Lq, H, 64), 31) * QK_C).half(), _rand((B, Lk, H, 64), 32).half(), _rand((B, Lk, H, 64), 33).half()
    out = torch.full((B, Lq, C), NAN, dtype=F16, device=dev)
    ops.attention(q.to(dev).view(B, Lq, C), k.to(dev).view(B, Lk, C), v.to(dev).view(B, Lk, C), out, nb0=B, nb1=1, heads=H, lq=Lq, lk=Lk,
                  q_strides=(Lq * C, 0, C), k_strides=(Lk * C, 0, C), o_strides=(Lq * C, 0, C), q_prescaled=True)
    r64 = _attn_r64(q, k, v, True).reshape(B, Lq, C)
    _check(_rounding_stats(out, r64, f"attention {case} ({B}, {H}, {Lq}, {Lk})"), case, same_ratio=False)


def test_c_attention_temporal(dev):
    """attn_kernel<1, 32>: tokens = frames (T = 21), batch = (b, pixel), read in place from [(b t), s, 3C]; 21 keys per row is where a
    biased rounding of P shows most (test_c_attention's docstring)."""
    from seva import ops
    B, T, S, H = 1, 21, 50, 2
    C = 64 * H
    qkv = _rand((B * T, S, 3 * C), 11).half()
    out = torch.full((B * T, S, C), NAN, dtype=F16, device=dev)
    qd = qkv.to(dev)
    ops.attention(qd[..., :C], qd[..., C:2 * C], qd[..., 2 * C:], out, nb0=B, nb1=S, heads=H, lq=T, lk=T,
                  q_strides=(T * S * 3 * C, 3 * C, S * 3 * C), k_strides=(T * S * 3 * C, 3 * C, S * 3 * C), o_strides=(T * S * C, C, S * C))
    x = qkv.view(B, T, S, 3, H, 64).permute(3, 0, 2, 4, 1, 5).double()  # [3, B, S, H, T, 64]
    r64 = torch.softmax(x[0] @ x[1].transpose(-1, -2) * 0.125, -1) @ x[2]
    r64 = r64.permute(0, 3, 1, 2, 4).reshape(B * T, S, C)
    _check(_rounding_stats(out, r64, f"attention temporal T={T} S={S} H={H}"), "temporal", same_ratio=False)


def test_c_attention_small(dev):
    from seva import ops
    B, H, L, D = 2, 16, 257, 80
    q, k, v = (_rand((B, L, H, D), s).half() for s in (41, 42, 43))
    out = torch.full((B, L, H * D), NAN, dtype=F16, device=dev)
    st = (L * H * D, H * D)
    ops.attention_small(q.to(dev).view(B, L, H * D), k.to(dev).view(B, L, H * D), v.to(dev).view(B, L, H * D), out, batch=B, heads=H, L=L,
                        head_dim=D, q_strides=st, k_strides=st, o_strides=st, scale=D ** -0.5)
    r64 = _attn_r64(q, k, v, False).reshape(B, L, H * D)
    _check(_rounding_stats(out, r64, f"attention_small ({B}, {H}, {L}, {D})"), "attention_small", same_ratio=False)
