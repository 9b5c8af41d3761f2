"""The opt-in fp8 VAE decoder on the GPU: the e4m3 window-conv instantiations it needs (csrc/conv_win.hip: 2-D tiles, fused
nearest-2x upsample, the e4m3 output epilogue `out_f8`) through `ops.conv3x3`, and the decoder itself (`AutoEncoder.set_precision`).

Convs are checked BIT-EXACTLY on integer data: small integers are exact in e4m3, the per-channel weight scales are powers of two
(the MFMA's E8M0 block scale), and every fp32 partial sum stays an exact dyadic number below 2^24 ulps -- outputs and GroupNorm
statistics then equal an fp64 reference in any reduction order."""
import warnings

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

U8 = torch.uint8


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from seva import _native
    _native.load()
    return torch.device("cuda:0")


def _ints(shape, lo, hi, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float64).to(dev)


def _up2(x):  # nearest-2x of an NHWC tensor
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2)


def _conv_ref(x, w, bias, res):
    """fp64 3x3 / pad 1 conv of NHWC x [n, h, w, cin] with w [cout, cin, 3, 3]: nine shifted GEMMs; -> [n, h * w, cout] (+ res)"""
    n, h, wd, cin = x.shape
    cout = w.shape[0]
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    out = bias.view(1, cout).expand(n * h * wd, cout).clone() + res.reshape(n * h * wd, cout)
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + h, kx:kx + wd, :].reshape(-1, cin) @ w[:, :, ky, kx].T
    return out.view(n, h * wd, cout)


def _case(dev, n, ih, iw, cin, cout, up, seed, wlo=-1, whi=1, scales=(-1, 0, 1)):
    """integer activations / weights exact in e4m3, power-of-two channel scales; returns e4m3 operands and the fp64 reference"""
    from seva import ops
    x = _ints((n, ih, iw, cin), -1, 1, dev, seed)
    w = _ints((cout, cin, 3, 3), wlo, whi, dev, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    e = torch.tensor(scales)[torch.randint(0, len(scales), (cout,), generator=g)].to(dev)
    ws = w * torch.exp2(e.double())[:, None, None, None]
    oh, ow = (2 * ih, 2 * iw) if up else (ih, iw)
    bias, res = _ints((cout,), -4, 4, dev, seed + 3), _ints((n, oh * ow, cout), -4, 4, dev, seed + 4)
    ref = _conv_ref(_up2(x) if up else x, ws, bias, res)
    x8 = ops.to_fp8(x)
    w8 = ops.to_fp8(w.permute(0, 2, 3, 1).reshape(cout, 9 * cin))
    return x8, w8, (e + 127).to(U8), bias.float(), res.float(), ref


# (n, ih, iw, cin, cout, upsample): the decoder's sides 72 / 144 / 288 / 576 (linear tiles at 72, 2-D tiles from 144), 128 / 256 / 512
# channels, plain and fused-upsample, one and three images, and non-square images (96 x 72 source, as a 768 x 576 frame decodes)
EXACT = [
    (1, 72, 72, 512, 512, False), (3, 72, 72, 512, 512, False), (1, 144, 144, 512, 512, False), (3, 144, 144, 256, 256, False),
    (1, 288, 288, 256, 256, False), (3, 288, 288, 128, 128, False), (1, 576, 576, 128, 128, False), (1, 288, 288, 512, 256, False),
    (3, 96, 72, 256, 128, False), (1, 192, 144, 128, 256, False),
    (1, 36, 36, 512, 512, True), (3, 72, 72, 512, 512, True), (1, 144, 144, 512, 512, True), (1, 288, 288, 256, 256, True),
    (3, 96, 72, 256, 256, True), (1, 72, 72, 128, 128, True),
]


@pytest.mark.parametrize("fam", [-1, 2], ids=["default", "8wave"])
@pytest.mark.parametrize("n,ih,iw,cin,cout,up", EXACT, ids=[f"{c[0]}x{c[1]}x{c[2]}x{c[3]}-{c[4]}{'-up' if c[5] else ''}" for c in EXACT])
def test_e4m3_window_conv_integer_exact(dev, n, ih, iw, cin, cout, up, fam, knobs):
    """Output and per-image channel statistics equal fp64 exactly, for the default (4-wave) and the 8-wave family (knob conv_win = 2);
    without upsample the result is bitwise the per-tap gather's."""
    from seva import ops
    x8, w8, e8, bias, res, ref = _case(dev, n, ih, iw, cin, cout, up, seed=ih * 7 + cin + cout + n + int(up))
    oh, ow = (2 * ih, 2 * iw) if up else (ih, iw)
    hw = oh * ow
    knobs(conv_win=fam)
    out = torch.full((n, hw, cout), float("nan"), device=dev)
    st = torch.full(ops.channel_stats_shape(n * hw, cout), float("nan"), device=dev)
    ops.conv3x3(x8, w8, w_exp=e8, upsample=up, bias=bias, residual=res, out_f32=out, ch_stats=st)
    torch.cuda.synchronize()
    assert torch.equal(out.double(), ref), f"max diff {(out.double() - ref).abs().max()}"
    blocks = st.double().view(n, hw // 64, 2, cout).sum(1)  # the blocks of an image add up to that image (any partition)
    assert torch.equal(blocks[:, 0], ref.sum(1)) and torch.equal(blocks[:, 1], (ref * ref).sum(1))
    if not up:
        knobs(conv_win=0)
        gat = torch.full((n, hw, cout), float("nan"), device=dev)
        ops.conv3x3(x8, w8, w_exp=e8, bias=bias, residual=res, out_f32=gat)
        torch.cuda.synchronize()
        assert torch.equal(out, gat)


# random data, cin >= 256: the window kernel reduces slab-outer / tap-inner, the per-tap gather tap-outer, so their fp32 sums round
# differently -- a plain e4m3 conv that fell back to the gather would show as bitwise equal to it.  Sides 72 (linear tiles) and 144 / 288 /
# 576 (2-D tiles), the decoder's channel counts, a non-square image
WINDOW = [(3, 72, 72, 512, 512), (1, 144, 144, 512, 512), (2, 288, 288, 256, 256), (1, 288, 288, 512, 256), (1, 576, 576, 256, 128),
          (2, 96, 72, 256, 128), (1, 192, 144, 256, 256)]


@pytest.mark.parametrize("n,ih,iw,cin,cout", WINDOW)
def test_plain_e4m3_conv_runs_the_window_kernel(dev, n, ih, iw, cin, cout, knobs):
    """The default dispatch, the 4-wave (conv_win = 1) and the 8-wave (2) family give the same bits (one reduction order), and those
    bits are NOT the per-tap gather's (conv_win = 0), which agrees only to fp32 rounding."""
    from seva import ops
    g = torch.Generator().manual_seed(ih + 3 * cin + cout)
    x8 = ops.to_fp8(torch.randn(n, ih, iw, cin, generator=g) * 2).to(dev)
    w8, e8 = ops.quantize_weight_fp8(torch.randn(cout, 9 * cin, generator=g) * 0.02)
    w8, e8 = w8.to(dev), e8.to(dev)
    bias, res = torch.randn(cout, generator=g).to(dev), torch.randn(n, ih * iw, cout, generator=g).to(dev)
    outs = {}
    for fam in (-1, 1, 2, 0):
        knobs(conv_win=fam)
        o = torch.full((n, ih * iw, cout), float("nan"), device=dev)
        ops.conv3x3(x8, w8, w_exp=e8, bias=bias, residual=res, out_f32=o)
        outs[fam] = o
    torch.cuda.synchronize()
    assert torch.isfinite(outs[-1]).all() and torch.equal(outs[-1], outs[1]) and torch.equal(outs[-1], outs[2])
    assert not torch.equal(outs[-1], outs[0])
    assert rel_l2(outs[-1], outs[0]) < 1e-5


@pytest.mark.parametrize("fam", [-1, 2], ids=["default", "8wave"])
@pytest.mark.parametrize("n,ih,iw,cin,cout", [(1, 36, 36, 512, 512), (3, 72, 72, 512, 512), (1, 144, 144, 256, 256), (2, 96, 72, 256, 128)])
def test_fused_upsample_equals_explicit_upsample(dev, n, ih, iw, cin, cout, fam, knobs):
    """Random e4m3 data: the conv with upsample=True is bitwise the same conv on the explicitly nearest-2x upsampled input."""
    from seva import ops
    g = torch.Generator().manual_seed(ih + cin)
    x8 = ops.to_fp8(torch.randn(n, ih, iw, cin, generator=g) * 2).to(dev)
    w8, e8 = ops.quantize_weight_fp8(torch.randn(cout, 9 * cin, generator=g) * 0.02)
    w8, e8 = w8.to(dev), e8.to(dev)
    bias, res = torch.randn(cout, generator=g).to(dev), torch.randn(n, 4 * ih * iw, cout, generator=g).to(dev)
    outs = []
    knobs(conv_win=fam)
    for xin, up in ((x8, True), (_up2(x8).contiguous(), False)):
        o = torch.full((n, 4 * ih * iw, cout), float("nan"), device=dev)
        ops.conv3x3(xin, w8, w_exp=e8, upsample=up, bias=bias, residual=res, out_f32=o)
        outs.append(o)
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("n,ih,iw,cin,cout", [(1, 72, 72, 512, 512), (3, 72, 72, 256, 256), (1, 144, 144, 512, 512), (3, 288, 288, 256, 256),
                                              (1, 96, 72, 128, 128)])
def test_out_f8_epilogue_is_saturating_rne_of_out_f32(dev, n, ih, iw, cin, cout, knobs):
    """Each out_f8 byte is torch's saturating RNE e4m3 cast of the same launch's out_f32 at that element (values reach well past
    +-448); out_f8 alone writes the same bytes; a wider pixel pitch leaves the pad bytes untouched."""
    from seva import ops
    x8, w8, e8, bias, res, ref = _case(dev, n, ih, iw, cin, cout, False, seed=5 * ih + cin, wlo=-3, whi=3, scales=(0, 1, 2, 3))
    hw = ih * iw
    assert ref.abs().max() > 2 * 448
    for fam in (-1, 2):
        knobs(conv_win=fam)
        out = torch.full((n, hw, cout), float("nan"), device=dev)
        o8 = torch.full((n, hw, cout + 8), 0x7F, dtype=U8, device=dev)
        ops.conv3x3(x8, w8, w_exp=e8, bias=bias, residual=res, out_f32=out, out_f8=o8[..., :cout])
        alone = torch.full((n, hw, cout), 0x7F, dtype=U8, device=dev)
        ops.conv3x3(x8, w8, w_exp=e8, bias=bias, residual=res, out_f8=alone)
        torch.cuda.synchronize()
        assert torch.equal(out.double(), ref)
        want = out.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(U8)
        assert torch.equal(o8[..., :cout], want), f"conv_win {fam}: {(o8[..., :cout] != want).sum().item()} bytes differ"
        assert bool((o8[..., cout:] == 0x7F).all()) and torch.equal(alone, want)
        sat = (out.abs() > 448.0)
        assert sat.any() and bool((o8[..., :cout][sat].view(torch.float8_e4m3fn).float().abs() == 448.0).all())


def test_fp8_conv_without_window_kernel_is_an_error(dev, knobs):
    """The per-tap gather has neither the fused upsample nor out_f8: where the window kernel does not run, the call raises."""
    from seva import ops
    from seva._native import SevaNativeError
    x8, w8, e8, bias, res, _ = _case(dev, 1, 16, 16, 128, 128, False, seed=9)
    out = torch.empty((1, 256, 128), device=dev)
    knobs(conv_win=0)
    with pytest.raises(SevaNativeError, match="window kernel"):
        ops.conv3x3(x8, w8, w_exp=e8, bias=bias, out_f8=torch.empty((1, 256, 128), dtype=U8, device=dev))
    with pytest.raises(SevaNativeError, match="window kernel"):
        ops.conv3x3(x8[:, :8, :8].contiguous(), w8, w_exp=e8, upsample=True, bias=bias, out_f32=out)


def test_upsample_with_out_f8_is_refused(dev, knobs):
    """No instantiation has both the fused upsample and the e4m3 output: the C-ABI refuses the pair (it must never report success without
    writing out_f8), and ops.conv3x3 asserts before the call."""
    import ctypes as C
    from seva import _native, ops
    from seva._native import SevaNativeError
    x8, w8, e8, bias, _, _ = _case(dev, 1, 16, 16, 128, 128, False, seed=10)
    src = x8[:, :8, :8].contiguous()
    o8 = torch.full((1, 256, 128), 0x7F, dtype=U8, device=dev)
    with pytest.raises(AssertionError):
        ops.conv3x3(src, w8, w_exp=e8, upsample=True, bias=bias, out_f8=o8)
    for fam in (-1, 0):
        knobs(conv_win=fam)
        d = _native.GemmDesc()
        d.a, d.w, d.bias, d.w_exp, d.out_f8, d.ldo8 = src.data_ptr(), w8.data_ptr(), bias.data_ptr(), e8.data_ptr(), o8.data_ptr(), 128
        d.M, d.N, d.K, d.lda = 256, 128, 9 * 128, 128
        d.mode, d.epilogue, d.rows_per_group = 1, 0, 1
        d.n, d.ih, d.iw, d.cin, d.oh, d.ow, d.stride, d.upsample = 1, 8, 8, 128, 16, 16, 1, 1
        with pytest.raises(SevaNativeError, match="out_f8 and the fused upsample"):
            _native.check(_native.load().seva_gemm_fp8(C.byref(d), _native.stream_ptr(dev)), "seva_gemm_fp8(conv)")
    torch.cuda.synchronize()
    assert bool((o8 == 0x7F).all())


# ------------------------------------------------------------------ the fp8 decoder


def _vae(dev, block_out=(128, 256, 512, 512), seed=3):
    from oracle import vae_ref as V
    from seva import synthetic as synth
    from seva.modules.autoencoder import AutoEncoder
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ae = AutoEncoder(random_init=True)
    ae.module.load_state_dict(synth.synth_state_dict(V.decoder_shapes(block_out=block_out), seed), strict=False)
    return ae.to(dev)


def _z(n, h, w, seed):
    return torch.randn(n, 4, h, w, generator=torch.Generator().manual_seed(seed)) * 0.18215 * 4


# (SEVA_VAE_FP8_UPSAMPLE, rel-L2 bound): the default fp8 decode, and the opt-in e4m3 upsample convs fed by the out_f8 epilogue.  Bounds:
# 2x the rel-L2 to the f16 decode measured on these weights; the default one at most 5e-2
UPSAMPLE = [("0", 5e-2), ("1", 1.4e-1)]


@pytest.mark.parametrize("up8", ["0", "1"])
def test_fp8_decode_is_batch_invariant(dev, up8, monkeypatch):
    monkeypatch.delenv("SEVA_VAE_PRECISION", raising=False)
    monkeypatch.setenv("SEVA_VAE_FP8_UPSAMPLE", up8)
    ae = _vae(dev).set_precision("fp8")
    z = _z(3, 72, 72, 11).to(dev)
    out3 = ae.decode(z)
    out1 = ae.decode(z[:1])
    torch.cuda.synchronize()
    assert (ae.engine().fp8_upsample, len(ae.engine().W8)) == ((True, 58) if up8 == "1" else (False, 52))
    assert torch.isfinite(out3).all() and torch.equal(out3[:1], out1)


@pytest.mark.parametrize("up8,bound", UPSAMPLE)
@pytest.mark.parametrize("n,h,w", [(7, 72, 72), (1, 96, 72)])
def test_fp8_decode_accuracy_vs_f16(dev, n, h, w, up8, bound, monkeypatch):
    """fp8 vs f16 decode of the same synthetic latent (576 x 576 x 7 frames; a 768 x 576 frame)."""
    monkeypatch.delenv("SEVA_VAE_PRECISION", raising=False)
    monkeypatch.setenv("SEVA_VAE_FP8_UPSAMPLE", up8)
    ae = _vae(dev)
    z = _z(n, h, w, 12).to(dev)
    ref = ae.set_precision("f16").decode(z)
    got = ae.set_precision("fp8").decode(z)
    torch.cuda.synchronize()
    err = rel_l2(got, ref)
    print(f"fp8 (e4m3 upsample {up8}) vs f16 VAE decode {n}x{h}x{w} latent: rel-L2 {err:.3e}")
    assert got.shape == ref.shape == (n, 3, 8 * h, 8 * w)
    assert err == err and err < bound


@pytest.mark.parametrize("up8", ["0", "1"])
def test_switching_back_to_f16_is_bitwise_default(dev, up8, monkeypatch):
    monkeypatch.delenv("SEVA_VAE_PRECISION", raising=False)
    monkeypatch.setenv("SEVA_VAE_FP8_UPSAMPLE", up8)
    z = _z(2, 24, 32, 13).to(dev)
    fresh = _vae(dev)
    assert fresh.precision == "f16"
    want = fresh.decode(z)
    ae = _vae(dev).set_precision("fp8")
    f8 = ae.decode(z)
    back = ae.set_precision("f16").decode(z)
    torch.cuda.synchronize()
    assert not torch.equal(f8, want) and torch.equal(back, want)
    assert ae.engine().W8 is not None  # packed once, kept
