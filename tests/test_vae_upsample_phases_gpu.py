"""The VAE decoders' upsample convs as four 2x2 phase convs on the source image, on the 128-column tiles of the window kernel
(`ops.conv3x3_up_phases128`, seva_gemm_desc.upsample = 4; csrc/conv_win.hip: PH with 2-D tiles and GroupNorm statistics), and the
decoder switch `AutoEncoder.set_upsample` / SEVA_VAE_UPSAMPLE_PHASES.  Run on the MI355X box: `python -m pytest tests -m gpu`.

Checks: bit-exact against torch on integer data for the default dispatch and both families, on linear tiles (whole-launch and
per-image) and 2-D tiles; the families agree bitwise on random data; a frame of a batch equals the frame alone; the error against
the fp64 conv on the fp32 weights is that of the nine-tap f16 path (e_phase <= 1.10 e_ninetap: two draws of the same f16
weight-rounding noise, asserted where the case is large enough for the ratio to be tight, printed otherwise); the statistics
blocks of an image add up to that image within the bound of a 64-term fp32 sum per block, exactly ceil(M_out / 64) blocks are
written, and a GroupNorm fed with them equals the one with its own statistics pass; everything the path does not compute raises
and writes nothing; the decoder takes the operator when asked, hands its statistics on, and returns to the default bits."""
import ctypes as C
import warnings

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


# n, ih, iw, cin, cout: the smallest shapes that reach each tiling
CASES = [
    (3, 8, 8, 64, 128),      # linear tiles over the whole launch: a 128-pixel tile straddles two images
    (2, 8, 72, 64, 128),     # per-image linear tiles: the window fits one image's tile, not a straddling one
    (2, 16, 144, 64, 128),   # 2-D tiles (16 x 8 source pixels; 16 x 16 in the 8-wave family)
    (1, 8, 96, 128, 256),    # 2-D tiles; 8 source rows: the 8-wave family's 16-row tile does not apply, knob 2 runs the 4-wave one
    (2, 16, 16, 128, 512),   # 512 channels
    (3, 5, 7, 64, 128),      # odd size, ih * iw % 64 != 0: no statistics
]
FAMILIES = (1, 2)  # conv_win knob: two 4-wave workgroups per CU on 128-row tiles / one 8-wave workgroup on a 256-row tile


def _nhwc(t, n, oh, ow, cout):
    return t.permute(0, 2, 3, 1).reshape(n, oh * ow, cout)


def _has_stats(ih, iw):
    return (ih * iw) % 64 == 0


def _stats_buffer(dev, n, ih, iw, cout):
    """NaN-filled, three blocks longer than the launch may write"""
    from seva import ops
    nb = ops.channel_stats_shape(n * 4 * ih * iw, cout)[0]
    return torch.full((nb + 3, 2, cout), float("nan"), device=dev), nb


def _check_stats(st, nb, out, n, ih, iw, cout, what):
    """Exactly the first ceil(M_out / 64) blocks are written; the hw_out / 64 blocks of image i sit in [i hw_out / 64, (i + 1) hw_out / 64)
    and add up to the image's fp64 sums of the STORED out_f32 within 64 * 2^-24 * sum |v| (sum v^2 for the squares): each block is a
    64-term fp32 sum, whose error is at most 63 roundings of partial sums that never exceed the block's sum of magnitudes."""
    assert bool(torch.isfinite(st[:nb]).all()) and bool(torch.isnan(st[nb:]).all()), what
    hw = 4 * ih * iw
    assert nb == n * hw // 64
    blocks = st[:nb].double().view(n, hw // 64, 2, cout).sum(1)
    o = out.double().view(n, hw, cout)
    s, q, sa = o.sum(1), (o * o).sum(1), o.abs().sum(1)
    u = 64 * 2.0 ** -24
    es, eq = (blocks[:, 0] - s).abs(), (blocks[:, 1] - q).abs()
    print(f"{what}: statistics max |sum err| / bound {float((es / (u * sa).clamp_min(1e-300)).max()):.3f}, "
          f"squares {float((eq / (u * q).clamp_min(1e-300)).max()):.3f}")
    assert bool((es <= u * sa).all()) and bool((eq <= u * q).all()), what


@pytest.mark.parametrize("n,ih,iw,cin,cout", CASES)
def test_phases128_exact_on_integers(dev, n, ih, iw, cin, cout, knobs):
    """Integer data (combined |w| <= 8: exact in f16, sums exact in fp32): bit-exact against torch for the default dispatch and both
    families, every output row written; statistics where ih * iw % 64 == 0."""
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
        st, nb = _stats_buffer(dev, n, ih, iw, cout) if _has_stats(ih, iw) else (None, 0)
        ops.conv3x3_up_phases128(xh, w4, bias=bias, out_f32=out, ch_stats=st, alg_k=9 * cin)
        assert torch.equal(out, ref), f"family {fam}: max diff {(out - ref).abs().max()}"
        if st is not None:
            _check_stats(st, nb, out, n, ih, iw, cout, f"integers {n}x{ih}x{iw} cin {cin} cout {cout} family {fam}")
    # without bias, without statistics
    knobs(conv_win=-1)
    out = torch.full((n, 4 * ih * iw, cout), float("nan"), device=dev)
    ops.conv3x3_up_phases128(xh, w4, out_f32=out)
    assert torch.equal(out, ref - bias)


@pytest.mark.parametrize("n,ih,iw,cin,cout", CASES)
def test_phases128_random_families_frames_error_and_statistics(dev, n, ih, iw, cin, cout, knobs):
    """Random data.  The families agree bitwise, output and statistics.  The last frame of a batch equals the frame alone, bitwise,
    in every family.  Error against the fp64 conv on the fp32 weights: e_phase <= 1.10 * e_ninetap (`ops.conv3x3(upsample=True)` on
    f16(w)), asserted with at least 1e5 output values and cin >= 128, printed otherwise.  Statistics as in `_check_stats`."""
    from seva import ops
    from seva._engine import combine_up_phases, pack_conv3x3
    x = _rand((n, ih, iw, cin), dev, 6).half()
    w = _rand((cout, cin, 3, 3), dev, 7, 0.05)
    bias = _rand((cout,), dev, 8)
    w4, w9 = combine_up_phases(w), pack_conv3x3(w)
    stats = _has_stats(ih, iw)
    outs = []
    for fam in (-1,) + FAMILIES:
        knobs(conv_win=fam)
        o = torch.full((n, 4 * ih * iw, cout), float("nan"), device=dev)
        st, nb = _stats_buffer(dev, n, ih, iw, cout) if stats else (None, 0)
        ops.conv3x3_up_phases128(x, w4, bias=bias, out_f32=o, ch_stats=st, alg_k=9 * cin)
        one = torch.full((1, 4 * ih * iw, cout), float("nan"), device=dev)
        st1, nb1 = _stats_buffer(dev, 1, ih, iw, cout) if stats else (None, 0)
        ops.conv3x3_up_phases128(x[-1:].contiguous(), w4, bias=bias, out_f32=one, ch_stats=st1, alg_k=9 * cin)
        assert torch.equal(one[0], o[-1]), f"family {fam}: the last frame differs from the frame alone"
        if stats:
            _check_stats(st, nb, o, n, ih, iw, cout, f"random {n}x{ih}x{iw} cin {cin} cout {cout} family {fam}")
            # within a family a frame's blocks hold the same pixels in the same order alone and in the batch: the same bits
            assert torch.equal(st1[:nb1], st[nb - nb1:nb]), f"family {fam}: the last frame's statistics differ from the frame alone"
        outs.append(o)
    assert torch.equal(outs[1], outs[2]), "the two families differ"
    assert torch.equal(outs[0], outs[1])
    knobs(conv_win=-1)
    o9 = torch.full((n, 4 * ih * iw, cout), float("nan"), device=dev)
    ops.conv3x3(x, w9, upsample=True, bias=bias, out_f32=o9)
    x64 = F.interpolate(x.permute(0, 3, 1, 2).double(), scale_factor=2, mode="nearest")
    ref64 = _nhwc(F.conv2d(x64, w.double(), bias.double(), padding=1), n, 2 * ih, 2 * iw, cout)
    e4, e9 = rel_l2(outs[0], ref64), rel_l2(o9, ref64)
    print(f"vae upsample phases {n}x{ih}x{iw} cin {cin} cout {cout}: e_phase {e4:.4e}  e_ninetap {e9:.4e}  ratio {e4 / e9:.4f}  "
          f"phases vs nine-tap {rel_l2(outs[0], o9):.3e}")
    assert e4 < 1e-3  # f16 weight rounding is 2^-11 / sqrt 3 = 2.8e-4 rms per weight; a wrong tap or phase would be O(1)
    if ref64.numel() >= 100000 and cin >= 128:
        assert e4 <= 1.10 * e9, (e4, e9)


@pytest.mark.parametrize("n,ih,iw,cin,cout", [c for c in CASES if _has_stats(c[1], c[2])])
def test_groupnorm_fed_with_phase_statistics(dev, n, ih, iw, cin, cout):
    """`seva_groupnorm` with the conv's statistics against its own statistics pass: the tolerance tests/test_ops_gpu.py uses for
    producer statistics (rel-L2 of the f16 outputs < 3e-4, and < 6e-4 to torch)."""
    from seva import ops
    from seva._engine import combine_up_phases
    x = _rand((n, ih, iw, cin), dev, 16).half()
    w4 = combine_up_phases(_rand((cout, cin, 3, 3), dev, 17, 0.05))
    hw = 4 * ih * iw
    out = torch.empty((n, hw, cout), device=dev)
    st = torch.empty(ops.channel_stats_shape(n * hw, cout), device=dev)
    ops.conv3x3_up_phases128(x, w4, bias=_rand((cout,), dev, 18), out_f32=out, ch_stats=st)
    gamma, beta = 1 + 0.1 * _rand((cout,), dev, 3), 0.1 * _rand((cout,), dev, 4)
    ws = ops.groupnorm_workspace(n, dev)
    o_pass = torch.empty((n, hw, cout), device=dev, dtype=torch.float16)
    o_st = torch.full_like(o_pass, float("nan"))
    ops.groupnorm(out, None, gamma, beta, o_pass, ws, eps=1e-6, silu=True)
    ops.groupnorm(out, None, gamma, beta, o_st, ws, eps=1e-6, silu=True, stats1=st)
    ref = F.silu(F.group_norm(out.transpose(1, 2), 32, gamma, beta, 1e-6).transpose(1, 2))
    e_st, e_two = rel_l2(o_st, ref), rel_l2(o_st, o_pass)
    print(f"groupnorm after phases {n}x{ih}x{iw} cout {cout}: producer statistics vs torch {e_st:.2e}, vs statistics pass {e_two:.2e}")
    assert e_st < 6e-4 and e_two < 3e-4


def _desc(x, w4, bias, out, cout, cin, n, ih, iw, up=4):
    from seva import _native
    d = _native.GemmDesc()
    d.a, d.w, d.bias, d.out_f32 = x.data_ptr(), w4.data_ptr(), bias.data_ptr(), out.data_ptr()
    d.M, d.N, d.K, d.lda, d.ldo32 = n * 4 * ih * iw, cout, 4 * cin, cin, cout
    d.mode, d.epilogue = 1, 0
    d.n, d.ih, d.iw, d.cin, d.oh, d.ow, d.stride, d.upsample = n, ih, iw, cin, 2 * ih, 2 * iw, 1, up
    return d


def test_phases128_refuses_what_it_does_not_compute(dev, knobs):
    """bias + out_f32 (+ ch_stats) only: residual, row_add, out_f16, out_f8, a2, split-K, col_scale, GEGLU, e4m3 operands,
    cout % 128 != 0, a wrong K, a shape neither tiling takes, statistics with ih * iw % 64 != 0 and a switched-off window kernel are
    errors (no other kernel reads the [4][N][4 cin] weights), and nothing is written.  Values 2 and 3 behave as before."""
    from seva import _native, ops
    from seva._native import SevaNativeError
    n, ih, iw, cin, cout = 1, 8, 8, 128, 128
    x = _rand((n, ih, iw, cin), dev, 1).half()
    w4 = _rand((4, cout, 4 * cin), dev, 2, 0.05).half()
    bias = _rand((cout,), dev, 3)
    out = torch.full((n, 4 * ih * iw, cout), 7.0, device=dev)
    other = torch.zeros((n, 4 * ih * iw, cout), device=dev)
    o16 = torch.zeros((n, 4 * ih * iw, cout), device=dev, dtype=torch.float16)
    o8 = torch.zeros((n, 4 * ih * iw, cout), device=dev, dtype=torch.uint8)
    st = torch.full((n * 4 * ih * iw // 64 + 1, 2, cout), 5.0, device=dev)
    lib = _native.load()

    def call(d, fn="seva_gemm_f16"):
        _native.check(getattr(lib, fn)(C.byref(d), _native.stream_ptr(dev)), fn)

    def base():
        return _desc(x, w4, bias, out, cout, cin, n, ih, iw)

    def residual(d): d.residual, d.ldr = other.data_ptr(), cout
    def row_add(d): d.row_add, d.rows_per_group = other.data_ptr(), 4 * ih * iw
    def out_f16(d): d.out_f16, d.ldo16 = o16.data_ptr(), cout
    def out_f8(d): d.out_f8, d.ldo8 = o8.data_ptr(), cout
    def a2(d): d.a2, d.lda2, d.K2 = o16.data_ptr(), cout, 128
    def splitk(d): d.splitk_ws, d.splitk_ws_bytes = other.data_ptr(), other.numel() * 4
    def col_scale(d): d.col_scale, d.col_scale_n = 0.5, 64
    def bad_k(d): d.K = 9 * cin
    def bad_n(d): d.N = 160
    def geglu(d): d.epilogue = 1

    for mutate in (residual, row_add, out_f16, out_f8, a2, splitk, col_scale, bad_k, bad_n, geglu):
        d = base()
        d.ch_stats = st.data_ptr()
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
    # a shape neither tiling takes: a 100-pixel source row is too long for the linear window and no multiple of 16
    xw = _rand((1, 8, 100, 64), dev, 4).half()
    ww = _rand((4, 128, 4 * 64), dev, 5, 0.05).half()
    ow_ = torch.full((1, 4 * 8 * 100, 128), 7.0, device=dev)
    with pytest.raises(SevaNativeError, match="window kernel"):
        ops.conv3x3_up_phases128(xw, ww, bias=bias, out_f32=ow_)
    # statistics where a 64-pixel block of one phase would leave its image
    xo = _rand((3, 5, 7, 64), dev, 6).half()
    oo = torch.full((3, 4 * 5 * 7, 128), 7.0, device=dev)
    so = torch.full((3 * 4 * 5 * 7 // 64 + 1, 2, 128), 5.0, device=dev)
    with pytest.raises(SevaNativeError, match="ch_stats"):
        ops.conv3x3_up_phases128(xo, ww, bias=bias, out_f32=oo, ch_stats=so)
    with pytest.raises(ValueError):
        ops.conv3x3_up_phases128(x, w4, bias=bias)
    knobs(conv_win=0)  # the window kernel switched off: an error, never the per-tap gather on these weights
    with pytest.raises(SevaNativeError, match="window kernel"):
        call(base())
    knobs(conv_win=-1)
    # values 2 and 3 as before: 2 is the 160-column family (refuses N = 128 and ch_stats), 3 is no value
    for up in (2, 3):
        with pytest.raises(SevaNativeError):
            call(_desc(x, w4, bias, out, cout, cin, n, ih, iw, up=up))
    torch.cuda.synchronize()
    for t, v in ((out, 7.0), (ow_, 7.0), (oo, 7.0), (st, 5.0), (so, 5.0)):
        assert bool((t == v).all())
    assert not bool(o16.any()) and not bool(o8.any()) and not bool(other.any())
    d = base()  # and the plain call runs
    d.ch_stats = st.data_ptr()
    call(d)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).any()) and not bool((st[:-1] == 5.0).any()) and bool((st[-1] == 5.0).all())


# ------------------------------------------------------------------ the decoder switch

FULL = (128, 256, 512, 512)


def _vae(dev, block_out=FULL, seed=3):
    from oracle import vae_ref as V
    from seva import synthetic as synth
    from seva.modules.autoencoder import AutoEncoder, VaeWeights
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ae = AutoEncoder(random_init=True)
    if tuple(block_out) != tuple(ae.module.block_out):
        ae.module = VaeWeights(block_out=block_out).eval().requires_grad_(False)
    sd = synth.synth_state_dict(V.decoder_shapes(block_out=block_out), seed)
    ae.module.load_state_dict(sd, strict=False)
    return ae.to(dev), sd


def _clean_env(monkeypatch):
    for k in ("SEVA_VAE_UPSAMPLE_PHASES", "SEVA_VAE_PRECISION", "SEVA_VAE_FP8_UPSAMPLE"):
        monkeypatch.delenv(k, raising=False)


def _spies(monkeypatch):
    """records of the decode's upsample convs: phase-operator calls (out pointer, statistics?), nine-tap upsample calls, and what
    statistics each GroupNorm input arrived with"""
    from seva import ops
    rec = {"phases": [], "taps": 0, "gn": {}}
    real_p, real_c, real_g = ops.conv3x3_up_phases128, ops.conv3x3, ops.groupnorm

    def phases(x, w4, **k):
        rec["phases"].append((k["out_f32"].data_ptr(), k.get("ch_stats") is not None))
        return real_p(x, w4, **k)

    def conv(x, w, **k):
        rec["taps"] += bool(k.get("upsample"))
        return real_c(x, w, **k)

    def gn(x1, *a, **k):
        rec["gn"][x1.data_ptr()] = k.get("stats1") is not None
        return real_g(x1, *a, **k)

    monkeypatch.setattr(ops, "conv3x3_up_phases128", phases)
    monkeypatch.setattr(ops, "conv3x3", conv)
    monkeypatch.setattr(ops, "groupnorm", gn)
    return rec


@pytest.fixture(scope="module")
def frame_64x192():
    """two 64 x 192 px frames (latent 8 x 24: upsample sources 8 x 24 and 16 x 48 on linear tiles, 32 x 96 on 2-D tiles) and their
    decode by oracle/vae_ref.py, computed once"""
    from oracle import vae_ref as V
    from seva import synthetic as synth
    z = torch.randn(2, 4, 8, 24, generator=torch.Generator().manual_seed(21)) * 0.18215 * 4
    sd = synth.synth_state_dict(V.decoder_shapes(block_out=FULL), 3)
    return z, V.vae_decode(sd, z)


@pytest.mark.parametrize("precision", ["f16", "fp8"])
def test_decoder_switch(dev, precision, frame_64x192, monkeypatch):
    """The default decode is the "taps" decode, bitwise, also after a "phases" decode; "phases" runs the three upsample convs through
    the new operator (none through `conv3x3(upsample=True)`) and each following GroupNorm receives their statistics; the error
    against oracle/vae_ref.py stays that of the nine-tap decode (e_phases <= 1.10 e_taps) and the two decodes do differ."""
    _clean_env(monkeypatch)
    z, ref = frame_64x192
    z = z.to(dev)
    fresh, _ = _vae(dev)
    default = fresh.set_precision(precision).decode(z)
    ae, _ = _vae(dev)
    ae.set_precision(precision)
    rec = _spies(monkeypatch)
    assert ae.upsample == "taps"
    got = ae.set_upsample("phases").decode(z)
    assert len(rec["phases"]) == 3 and rec["taps"] == 0
    for ptr_, with_stats in rec["phases"]:
        assert with_stats and rec["gn"].get(ptr_) is True  # the GroupNorm that reads the conv's output got its statistics
    assert set(ae.engine().W4) == {f"decoder.up_blocks.{i}.upsamplers.0.conv.w4" for i in range(3)}
    rec["phases"].clear()
    taps = ae.set_upsample("taps").decode(z)
    assert not rec["phases"] and rec["taps"] == 3
    torch.cuda.synchronize()
    assert torch.equal(taps, default)
    e_ph, e_tp, d = rel_l2(got.cpu(), ref), rel_l2(taps.cpu(), ref), rel_l2(got, taps)
    print(f"vae decode 64x192 x2 ({precision}): phases vs oracle {e_ph:.3e}, taps vs oracle {e_tp:.3e}, phases vs taps {d:.3e}")
    assert got.shape == (2, 3, 64, 192) and 0 < d
    assert e_ph <= 1.10 * e_tp, (e_ph, e_tp)


def test_env_switch_is_read_at_engine_build(dev, frame_64x192, monkeypatch):
    _clean_env(monkeypatch)
    z = frame_64x192[0][:1].to(dev)
    monkeypatch.setenv("SEVA_VAE_UPSAMPLE_PHASES", "1")
    ae, _ = _vae(dev)
    rec = _spies(monkeypatch)
    by_env = ae.decode(z)
    assert len(rec["phases"]) == 3 and rec["taps"] == 0
    monkeypatch.delenv("SEVA_VAE_UPSAMPLE_PHASES")
    other, _ = _vae(dev)
    by_method = other.set_upsample("phases").decode(z)
    assert torch.equal(by_env, by_method)


def test_narrow_decoder_keeps_the_nine_taps_where_the_tiles_do_not_fit(dev, monkeypatch):
    """block_out = (64, 64, 128, 128): the two 128-channel upsample convs take the operator, the 64-channel one stays nine-tap, and
    the decode still matches the oracle."""
    from oracle import vae_ref as V
    _clean_env(monkeypatch)
    ae, sd = _vae(dev, (64, 64, 128, 128))
    z = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(5)) * 0.18215 * 4
    rec = _spies(monkeypatch)
    out = ae.set_upsample("phases").decode(z.to(dev))
    assert len(rec["phases"]) == 2 and rec["taps"] == 1
    err = rel_l2(out.cpu(), V.vae_decode(sd, z))
    print(f"narrow vae decode with phases: rel-L2 {err:.3e}")
    assert out.shape == (2, 3, 64, 64) and err < 2e-3
