"""The Upsample convs of a step as four 2x2 phase convs on the source image (`ops.conv3x3_up_phases`, seva_gemm_desc.upsample = 2;
reference seva/modules/layers.py:35-46: nearest-2x, then conv3x3).  Output rows 2i and 2i + 1 read source rows {i-1, i, i} and
{i, i, i+1}, columns alike, so each output phase (py, px) is a 2x2 conv with summed weights (`seva._engine.combine_up_phases`):
4 taps instead of 9.  Run on the MI355X box: `python -m pytest tests -m gpu`.

Checks: bit-exact against torch on integer data for both instantiation families; the families agree bitwise on random data; a frame
of a batch equals the frame alone; the error against the fp64 conv on the fp32 weights is that of the nine-tap f16 path (two
independent draws of the same f16 weight-rounding noise: e4 <= 1.10 e9, asserted where the case is large enough for the ratio of
two noise draws to be tight, printed otherwise); every combination the path does not compute raises."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from conftest import rel_l2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from seva import _native
    _native.load()
    return torch.device("cuda:0")


def _ints(shape, lo, hi, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float().to(dev)


def _rand(shape, dev, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev)


# n, ih, iw, cin, cout: the three shapes of a 576 x 576 step at small batch (36 -> 72 at 640 channels, 18 -> 36 and 9 -> 18 at 1280), odd and
# non-square sizes, the 9 x 9 level at the CFG batch of 42 (tiles that straddle images), a 72-px-wide source (per-image tiles)
CASES = [
    (2, 36, 36, 640, 640), (2, 18, 18, 1280, 1280), (3, 9, 9, 1280, 1280),
    (5, 7, 5, 128, 160), (1, 16, 24, 192, 320), (3, 5, 7, 64, 160),
    (42, 9, 9, 128, 320), (2, 72, 72, 64, 160),
]
FAMILIES = (1, 2)  # conv_win knob: two 4-wave workgroups per CU on 160-row tiles / one 8-wave workgroup on a 256-row tile


def _nhwc(t, n, oh, ow, cout):
    return t.permute(0, 2, 3, 1).reshape(n, oh * ow, cout)


@pytest.mark.parametrize("n,ih,iw,cin,cout", CASES)
def test_phases_exact_on_integers(dev, n, ih, iw, cin, cout, knobs):
    """Integer data (combined |w| <= 8: exact in f16, sums exact in fp32): bit-exact against torch, for the default dispatch and
    both families."""
    from seva import ops
    from seva._engine import combine_up_phases
    x = _ints((n, cin, ih, iw), -3, 3, dev, 1)
    w = _ints((cout, cin, 3, 3), -2, 2, dev, 2)
    bias = _ints((cout,), -4, 4, dev, 3)
    ref = _nhwc(F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, bias, padding=1), n, 2 * ih, 2 * iw, cout)
    xh, w4 = x.permute(0, 2, 3, 1).contiguous().half(), combine_up_phases(w)
    for fam in (-1,) + FAMILIES:
        knobs(conv_win=fam)
        out = torch.full((n, 4 * ih * iw, cout), float("nan"), device=dev)
        ops.conv3x3_up_phases(xh, w4, bias=bias, out_f32=out, alg_k=9 * cin)
        assert torch.equal(out, ref), f"family {fam}: max diff {(out - ref).abs().max()}"
    # without bias
    knobs(conv_win=-1)
    out = torch.full((n, 4 * ih * iw, cout), float("nan"), device=dev)
    ops.conv3x3_up_phases(xh, w4, out_f32=out)
    assert torch.equal(out, ref - bias)


@pytest.mark.parametrize("n,ih,iw,cin,cout", CASES)
def test_phases_random_families_frames_and_error(dev, n, ih, iw, cin, cout, knobs):
    """Random data.  The two families agree bitwise (which one runs may depend on the batch).  One frame of a batch equals the
    frame alone, bitwise, in every family.  Error against the fp64 conv on the fp32 weights: e4 (this path) <= 1.10 * e9 (the
    nine-tap f16 path on f16(w)); the 10 % is the sampling spread of two independent rounding draws, asserted on cases with at
    least 1e5 output values and cin >= 128, printed on the smaller ones."""
    from seva import ops
    from seva._engine import combine_up_phases, pack_conv3x3
    x = _rand((n, ih, iw, cin), dev, 6).half()
    w = _rand((cout, cin, 3, 3), dev, 7, 0.05)
    bias = _rand((cout,), dev, 8)
    w4, w9 = combine_up_phases(w), pack_conv3x3(w)
    outs = []
    for fam in (-1,) + FAMILIES:
        knobs(conv_win=fam)
        o = torch.full((n, 4 * ih * iw, cout), float("nan"), device=dev)
        ops.conv3x3_up_phases(x, w4, bias=bias, out_f32=o, alg_k=9 * cin)
        one = torch.full((1, 4 * ih * iw, cout), float("nan"), device=dev)
        ops.conv3x3_up_phases(x[-1:].contiguous(), w4, bias=bias, out_f32=one, alg_k=9 * cin)
        assert torch.equal(one[0], o[-1]), f"family {fam}: the last frame differs from the frame alone"
        outs.append(o)
    assert torch.equal(outs[1], outs[2]), "the two families differ"
    assert torch.equal(outs[0], outs[1])
    knobs(conv_win=-1)
    o9 = torch.full((n, 4 * ih * iw, cout), float("nan"), device=dev)
    ops.conv3x3(x, w9, upsample=True, bias=bias, out_f32=o9)
    x64 = F.interpolate(x.permute(0, 3, 1, 2).double(), scale_factor=2, mode="nearest")
    ref64 = _nhwc(F.conv2d(x64, w.double(), bias.double(), padding=1), n, 2 * ih, 2 * iw, cout)
    e4, e9 = rel_l2(outs[0], ref64), rel_l2(o9, ref64)
    print(f"upsample phases {n}x{ih}x{iw} cin {cin} cout {cout}: e4 {e4:.4e}  e9 {e9:.4e}  e4/e9 {e4 / e9:.4f}  "
          f"phases vs nine-tap {rel_l2(outs[0], o9):.3e}")
    if ref64.numel() >= 100000 and cin >= 128:
        assert e4 <= 1.10 * e9, (e4, e9)


def _desc(dev, x, w4, bias, out, cout, cin, n, ih, iw):
    from seva import _native
    d = _native.GemmDesc()
    d.a, d.w, d.bias, d.out_f32 = x.data_ptr(), w4.data_ptr(), bias.data_ptr(), out.data_ptr()
    d.M, d.N, d.K, d.lda, d.ldo32 = n * 4 * ih * iw, cout, 4 * cin, cin, cout
    d.mode, d.epilogue = 1, 0
    d.n, d.ih, d.iw, d.cin, d.oh, d.ow, d.stride, d.upsample = n, ih, iw, cin, 2 * ih, 2 * iw, 1, 2
    return d


def test_phases_refuses_what_it_does_not_compute(dev, knobs):
    """bias + out_f32 only.  residual, row_add, out_f16, a2, split-K, statistics, e4m3 operands, cout % 160 != 0, a wrong K and a
    switched-off window kernel are errors (no other kernel reads the [4][N][4 cin] weights), and nothing is written."""
    from seva import _native, ops
    from seva._native import SevaNativeError
    n, ih, iw, cin, cout = 1, 8, 8, 128, 160
    x = _rand((n, ih, iw, cin), dev, 1).half()
    w4 = _rand((4, cout, 4 * cin), dev, 2, 0.05).half()
    bias = _rand((cout,), dev, 3)
    out = torch.full((n, 4 * ih * iw, cout), 7.0, device=dev)
    other = torch.zeros((n, 4 * ih * iw, cout), device=dev)
    o16 = torch.zeros((n, 4 * ih * iw, cout), device=dev, dtype=torch.float16)
    lib = _native.load()

    def call(d, fn="seva_gemm_f16"):
        _native.check(getattr(lib, fn)(C.byref(d), _native.stream_ptr(dev)), fn)

    def base():
        return _desc(dev, x, w4, bias, out, cout, cin, n, ih, iw)

    def residual(d): d.residual, d.ldr = other.data_ptr(), cout
    def row_add(d): d.row_add, d.rows_per_group = other.data_ptr(), 4 * ih * iw
    def out_f16(d): d.out_f16, d.ldo16 = o16.data_ptr(), cout
    def a2(d): d.a2, d.lda2, d.K2 = o16.data_ptr(), cout, 128
    def splitk(d): d.splitk_ws, d.splitk_ws_bytes = other.data_ptr(), other.numel() * 4
    def stats(d): d.ch_stats = other.data_ptr()
    def bad_k(d): d.K = 9 * cin
    def bad_n(d): d.N = 128
    def geglu(d): d.epilogue = 1

    for mutate in (residual, row_add, out_f16, a2, splitk, stats, bad_k, bad_n, geglu):
        d = base()
        mutate(d)
        with pytest.raises(SevaNativeError):
            call(d)
    d = base()
    d.out_f32 = None
    d.out_f16, d.ldo16 = o16.data_ptr(), cout
    with pytest.raises(SevaNativeError):
        call(d)
    d = base()
    d.w_exp = bias.data_ptr()
    with pytest.raises(SevaNativeError):
        call(d, "seva_gemm_fp8")
    d = base()
    d.upsample = 3
    with pytest.raises(SevaNativeError):
        call(d)
    knobs(conv_win=0)  # the window kernel switched off: an error, never the per-tap gather on these weights
    with pytest.raises(SevaNativeError, match="window kernel"):
        call(base())
    knobs(conv_win=-1)
    with pytest.raises(ValueError):
        ops.conv3x3_up_phases(x, w4, bias=bias, out_f32=out, ch_stats=other)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and not bool(o16.any())
    call(base())  # and the plain call runs
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).all())


def test_engine_takes_the_phase_path_by_default(dev, monkeypatch):
    """`_resample` of the UNet engine: the phase operator by default, the nine-tap call with SEVA_UPSAMPLE_PHASES=0 (decided at call
    time); the two results differ by f16 weight rounding only, and the phase path hands no statistics to the consumer."""
    from seva import _engine, ops
    calls = []
    real = ops.conv3x3_up_phases
    monkeypatch.setattr(ops, "conv3x3_up_phases", lambda *a, **k: (calls.append(k.get("alg_k")), real(*a, **k))[1])

    class Spec:
        kind, prefix, channels = "up", "up0", 320

    eng = _engine.SevaEngine.__new__(_engine.SevaEngine)
    w = _rand((320, 320, 3, 3), dev, 4, 0.03)
    eng.W = {"up0.w": _engine.pack_conv3x3(w), "up0.w4": _engine.combine_up_phases(w), "up0.b": _rand((320,), dev, 5)}
    eng.gn_fused_stats = 1
    bufs = {}
    eng._buf = lambda name, shape, dtype, zero=False: bufs.setdefault((name, tuple(shape), dtype), torch.zeros(tuple(shape), dtype=dtype, device=dev))
    x = _engine.Act(_rand((2, 16 * 16, 320), dev, 6), 2, 16, 16)
    monkeypatch.delenv("SEVA_UPSAMPLE_PHASES", raising=False)
    o = eng._resample(Spec, x)
    o4 = o.t.clone()
    assert calls == [9 * 320] and (o.h, o.w) == (32, 32) and o.stats is None
    monkeypatch.setenv("SEVA_UPSAMPLE_PHASES", "0")
    o9 = eng._resample(Spec, x)
    assert calls == [9 * 320] and o9.stats is not None  # the nine-tap conv emits the statistics (hw = 1024)
    err = rel_l2(o4, o9.t)
    print(f"engine _resample 16 -> 32, 320 ch: phases vs nine-tap rel-L2 {err:.3e}")
    assert 0 < err < 1e-3
