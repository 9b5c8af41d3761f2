"""The opt-in fp8 VAE encoder on the GPU: the e4m3 stride-2, bottom/right-padded window conv (csrc/conv_win.hip, S2 instantiations)
through `ops.conv3x3`, and the encoder itself (`AutoEncoder.set_precision(..., encode="fp8")`).

Convs are checked BIT-EXACTLY on integer data, as in test_vae_fp8_gpu.py: small integers are exact in e4m3, the per-channel weight
scales are powers of two, and every fp32 partial sum stays an exact dyadic number, so outputs and GroupNorm statistics equal an fp64
reference in any reduction order.

By default the stride-2 e4m3 convs run on the per-tap gather (measured faster on the encoder's shapes); the conv_win knob (1 or 2) selects
the stride-2 window family, which must then run or raise."""
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


def _out_hw(ih, iw):
    return (ih - 2) // 2 + 1, (iw - 2) // 2 + 1


def _conv_s2_ref(x, w, bias, res):
    """fp64 3x3 / stride 2 conv of NHWC x [n, h, w, cin] padded (0, 1, 0, 1) (diffusers Downsample2D); -> [n, oh * ow, cout] (+ res)"""
    n, h, wd, cin = x.shape
    cout = w.shape[0]
    oh, ow = _out_hw(h, wd)
    xp = torch.nn.functional.pad(x, (0, 0, 0, 1, 0, 1))
    out = bias.view(1, cout).expand(n * oh * ow, cout).clone() + res.reshape(n * oh * ow, cout)
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + 2 * oh:2, kx:kx + 2 * ow:2, :].reshape(-1, cin) @ w[:, :, ky, kx].T
    return out.view(n, oh * ow, cout)


def _case(dev, n, ih, iw, cin, cout, seed):
    from seva import ops
    x = _ints((n, ih, iw, cin), -1, 1, dev, seed)
    w = _ints((cout, cin, 3, 3), -1, 1, dev, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    e = torch.tensor((-1, 0, 1))[torch.randint(0, 3, (cout,), generator=g)].to(dev)
    ws = w * torch.exp2(e.double())[:, None, None, None]
    oh, ow = _out_hw(ih, iw)
    bias, res = _ints((cout,), -4, 4, dev, seed + 3), _ints((n, oh * ow, cout), -4, 4, dev, seed + 4)
    ref = _conv_s2_ref(x, ws, bias, res)
    x8 = ops.to_fp8(x)
    w8 = ops.to_fp8(w.permute(0, 2, 3, 1).reshape(cout, 9 * cin))
    return x8, w8, (e + 127).to(U8), bias.float(), res.float(), ref


def _blocks_2d(ref, oh, ow):
    """GroupNorm statistics blocks of the 2-D tiles: tiles of 16 x 8 output pixels in row-major tile order, two 4-row blocks per tile"""
    n, _, c = ref.shape
    r = ref.view(n, oh // 8, 2, 4, ow // 16, 16, c).permute(0, 1, 4, 2, 3, 5, 6).reshape(n, -1, 64, c)
    return torch.stack((r.sum(2), (r * r).sum(2)), 2)


def _blocks_linear(ref):
    n, hw, c = ref.shape
    r = ref.view(n, hw // 64, 64, c)
    return torch.stack((r.sum(2), (r * r).sum(2)), 2)


# (n, ih, iw, cin, cout, family): linear tiles where one image's windows fit (output rows up to 72 px), 2-D tiles of 16 x 8 output
# pixels otherwise; the encoder's three downsample shapes at 576 x 576: 288 and 144 px outputs on 2-D tiles, 72 px on linear tiles
EXACT = [(n, ih, iw, c, c, "lin") for n in (1, 3) for (ih, iw) in ((16, 16), (18, 18), (40, 24)) for c in (128, 256)] + [
    (3, 32, 24, 128, 128, "lin"), (2, 160, 160, 256, 256, "2d"),
    (1, 576, 576, 128, 128, "2d"), (1, 288, 288, 256, 256, "2d"), (1, 144, 144, 512, 512, "lin"),
]


@pytest.mark.parametrize("stats", [False, True], ids=["nostats", "stats"])
@pytest.mark.parametrize("n,ih,iw,cin,cout,fam", EXACT, ids=[f"{c[0]}x{c[1]}x{c[2]}x{c[3]}-{c[5]}" for c in EXACT])
def test_e4m3_stride2_conv_integer_exact(dev, n, ih, iw, cin, cout, fam, stats, knobs):
    """Output equals fp64 exactly, on the window family (conv_win = 1) and on the default dispatch (the gather); with statistics (where
    oh * ow % 64 == 0) every 64-pixel block equals fp64, block by block in the partition of the window family that ran (64 consecutive
    rows: linear tiles; 4 x 16 pixel blocks in tile order: 2-D tiles)."""
    from seva import ops
    oh, ow = _out_hw(ih, iw)
    hw = oh * ow
    if stats and hw % 64:
        pytest.skip("statistics need oh * ow % 64 == 0 (the refusal is tested below)")
    x8, w8, e8, bias, res, ref = _case(dev, n, ih, iw, cin, cout, seed=ih * 7 + iw + cin + n)
    for knob in (1, -1):
        knobs(conv_win=knob)
        out = torch.full((n, hw, cout), float("nan"), device=dev)
        st = torch.full(ops.channel_stats_shape(n * hw, cout), float("nan"), device=dev) if stats else None
        ops.conv3x3(x8, w8, w_exp=e8, stride=2, pad_br_only=True, bias=bias, residual=res, out_f32=out, ch_stats=st)
        torch.cuda.synchronize()
        assert torch.equal(out.double(), ref), f"conv_win {knob}: max diff {(out.double() - ref).abs().max()}"
        if stats:
            want = _blocks_linear(ref) if fam == "lin" or knob == -1 else _blocks_2d(ref, oh, ow)
            assert torch.equal(st.double().view(n, hw // 64, 2, cout), want)


# random data, cin >= 256: the window kernel reduces slab-outer / tap-inner, the per-tap gather tap-outer; a stride-2 e4m3 conv that ran
# on the gather would be bitwise equal to it
WINDOW = [(3, 40, 24, 256, 256), (1, 144, 144, 512, 512), (1, 288, 288, 256, 256), (2, 160, 160, 512, 512)]


@pytest.mark.parametrize("n,ih,iw,cin,cout", WINDOW)
def test_e4m3_stride2_conv_runs_the_window_kernel(dev, n, ih, iw, cin, cout, knobs):
    from seva import ops
    g = torch.Generator().manual_seed(ih + 3 * cin + cout)
    oh, ow = _out_hw(ih, iw)
    x8 = ops.to_fp8(torch.randn(n, ih, iw, cin, generator=g) * 2).to(dev)
    w8, e8 = ops.quantize_weight_fp8(torch.randn(cout, 9 * cin, generator=g) * 0.02)
    w8, e8 = w8.to(dev), e8.to(dev)
    bias, res = torch.randn(cout, generator=g).to(dev), torch.randn(n, oh * ow, cout, generator=g).to(dev)
    outs = {}
    for fam in (1, 2, 0, -1):
        knobs(conv_win=fam)
        o = torch.full((n, oh * ow, cout), float("nan"), device=dev)
        ops.conv3x3(x8, w8, w_exp=e8, stride=2, pad_br_only=True, bias=bias, residual=res, out_f32=o)
        outs[fam] = o
    torch.cuda.synchronize()
    assert torch.isfinite(outs[1]).all() and torch.equal(outs[1], outs[2])  # knob 1 and 2: the one stride-2 window family
    assert torch.equal(outs[-1], outs[0])  # the default dispatch is the gather (measured faster)
    assert not torch.equal(outs[1], outs[0])
    assert rel_l2(outs[1], outs[0]) < 1e-5


def test_e4m3_stride2_conv_declined_is_an_error(dev, knobs):
    """With the window family asked for, shapes it declines raise instead of falling back to the gather: statistics over images with
    oh * ow % 64 != 0, an image too wide for the linear tiles whose output width is not a multiple of 16, the e4m3 output epilogue."""
    from seva import ops
    from seva._native import SevaNativeError
    knobs(conv_win=1)
    x8, w8, e8, bias, _, _ = _case(dev, 1, 18, 18, 128, 128, seed=21)
    out = torch.empty((1, 81, 128), device=dev)
    st = torch.empty(ops.channel_stats_shape(81, 128), device=dev)
    with pytest.raises(SevaNativeError, match="window kernel"):
        ops.conv3x3(x8, w8, w_exp=e8, stride=2, pad_br_only=True, bias=bias, out_f32=out, ch_stats=st)
    wide = ops.to_fp8(torch.ones(1, 402, 402, 128, device=dev))
    with pytest.raises(SevaNativeError, match="window kernel"):
        ops.conv3x3(wide, w8, w_exp=e8, stride=2, pad_br_only=True, bias=bias, out_f32=torch.empty((1, 200 * 200, 128), device=dev))
    with pytest.raises(SevaNativeError, match="window kernel"):
        ops.conv3x3(x8[:, :16, :16].contiguous(), w8, w_exp=e8, stride=2, pad_br_only=True, bias=bias,
                    out_f8=torch.empty((1, 64, 128), dtype=U8, device=dev))


# ------------------------------------------------------------------ the fp8 encoder


def _vae(dev, seed=3):
    from oracle import vae_ref as V
    from seva import synthetic as synth
    from seva.modules.autoencoder import AutoEncoder
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ae = AutoEncoder(random_init=True)
    ae.module.load_state_dict(synth.synth_state_dict({**V.decoder_shapes(), **V.encoder_shapes()}, seed))
    return ae.to(dev)


def _x(n, h, w, seed):
    return torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(seed)) * 2 - 1


@pytest.mark.parametrize("knob", [-1, 1], ids=["default", "s2window"])
@pytest.mark.parametrize("dn8", ["0", "1"])
def test_fp8_encode_is_batch_invariant(dev, dn8, knob, monkeypatch, knobs):
    """320 x 320 frames; with the stride-2 window family (conv_win = 1) the e4m3 downsample convs run 320 -> 160 and 160 -> 80 on 2-D
    tiles, 80 -> 40 on linear tiles."""
    knobs(conv_win=knob)
    monkeypatch.delenv("SEVA_VAE_ENCODE_PRECISION", raising=False)
    monkeypatch.setenv("SEVA_VAE_FP8_DOWNSAMPLE", dn8)
    ae = _vae(dev).set_precision("f16", encode="fp8")
    x = _x(3, 320, 320, 11).to(dev)
    z3 = ae.encode(x)
    z1 = [ae.encode(x[i:i + 1]) for i in range(3)]
    torch.cuda.synchronize()
    assert (ae.encoder_engine().fp8_downsample, len(ae.encoder_engine().W8)) == ((True, 42) if dn8 == "1" else (False, 36))
    assert torch.isfinite(z3).all() and all(torch.equal(z3[i:i + 1], z1[i]) for i in range(3))


# (SEVA_VAE_FP8_DOWNSAMPLE, rel-L2 bound): about 1.5x the largest rel-L2 of the fp8 encode to the f16 one measured on these weights at
# 64 / 144 / 576 px (8.9e-2 / 1.15e-1, both at 64 px)
DOWNSAMPLE = [("0", 1.4e-1), ("1", 1.8e-1)]


@pytest.mark.parametrize("dn8,bound", DOWNSAMPLE)
@pytest.mark.parametrize("n,h,w", [(2, 64, 64), (2, 144, 144), (1, 576, 576)])
def test_fp8_encode_accuracy_vs_f16(dev, n, h, w, dn8, bound, monkeypatch):
    monkeypatch.delenv("SEVA_VAE_ENCODE_PRECISION", raising=False)
    monkeypatch.setenv("SEVA_VAE_FP8_DOWNSAMPLE", dn8)
    ae = _vae(dev)
    x = _x(n, h, w, 12).to(dev)
    ref = ae.encode(x)
    got = ae.set_precision("f16", encode="fp8").encode(x)
    torch.cuda.synchronize()
    err = rel_l2(got, ref)
    print(f"fp8 (e4m3 downsample {dn8}) vs f16 VAE encode {n}x{h}x{w}: rel-L2 {err:.3e}")
    assert got.shape == ref.shape == (n, 4, h // 8, w // 8)
    assert err == err and err < bound


@pytest.mark.parametrize("dn8", ["0", "1"])
def test_fp8_encode_error_downstream_in_replace_channels(dev, dn8, monkeypatch):
    """What the encode error does to one denoiser call (tiny net, smoke()'s set-up): the input frame's latents in the `replace` channels
    come from the fp8 or the f16 encode of the same 128 x 128 image."""
    from seva import sampling as S
    from seva import synthetic as synth
    from seva.model import SGMWrapper, Seva, SevaParams
    monkeypatch.delenv("SEVA_VAE_ENCODE_PRECISION", raising=False)
    monkeypatch.setenv("SEVA_VAE_FP8_DOWNSAMPLE", dn8)
    ae = _vae(dev)
    img = _x(1, 128, 128, 14).to(dev)
    lat = {"f16": ae.encode(img), "fp8": ae.set_precision("f16", encode="fp8").encode(img)}
    T, hw = 3, 16
    params = SevaParams(model_channels=64)
    with torch.device("meta"):
        net = Seva(params)
    sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 0)
    net.load_state_dict(sd, strict=True, assign=True)
    net = net.to(dev).eval()
    sc = synth.synth_scene(T, (hw, hw), (0,), seed=7)
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(T, 4, hw, hw, generator=g) * 10).to(dev)
    sigma = torch.full((T,), 9.3527, device=dev)
    den = S.DiscreteDenoiser(S.DDPMDiscretization(), num_idx=1000, device=dev)
    outs = {}
    for k, z in lat.items():
        cond = {c: v.to(dev) for c, v in sc["cond"].items()}
        uc = {c: v.to(dev) for c, v in sc["uc"].items()}
        cond["replace"][0, :4] = z[0]
        with torch.no_grad():
            outs[k] = den(SGMWrapper(net), *S.MultiviewCFG(1.2).prepare_inputs(x, sigma, cond, uc), num_frames=T)
    torch.cuda.synchronize()
    e_lat, e_den = rel_l2(lat["fp8"], lat["f16"]), rel_l2(outs["fp8"], outs["f16"])
    print(f"fp8 (e4m3 downsample {dn8}) vs f16 encode: latents rel-L2 {e_lat:.3e}, one denoiser call on them {e_den:.3e}")
    assert torch.isfinite(outs["fp8"]).all() and 0.0 < e_den < 3e-3  # measured 1.1e-3 / 1.4e-3


@pytest.mark.parametrize("dn8", ["0", "1"])
def test_defaults_and_switching_back_are_bitwise_f16(dev, dn8, monkeypatch):
    """A default AutoEncoder encodes like one switched to fp8 and back; `set_precision("fp8")` alone (fp8 decode) leaves the encode
    f16, and its decode is bitwise that of an instance whose encode precision was never touched."""
    monkeypatch.delenv("SEVA_VAE_PRECISION", raising=False)
    monkeypatch.delenv("SEVA_VAE_ENCODE_PRECISION", raising=False)
    monkeypatch.setenv("SEVA_VAE_FP8_DOWNSAMPLE", dn8)
    x = _x(2, 64, 96, 15).to(dev)
    fresh = _vae(dev)
    assert fresh.encode_precision == "f16"
    want = fresh.encode(x)
    ae = _vae(dev).set_precision("f16", encode="fp8")
    z8 = ae.encode(x)
    back = ae.set_precision("f16", encode="f16").encode(x)
    torch.cuda.synchronize()
    assert not torch.equal(z8, want) and torch.equal(back, want)
    assert ae.encoder_engine().W8 is not None  # packed once, kept
    dec8 = _vae(dev).set_precision("fp8")
    assert dec8.encode_precision == "f16" and torch.equal(dec8.encode(x), want)
    z = want * 1.0
    both = ae.set_precision("fp8", encode="fp8")
    assert torch.equal(both.decode(z), dec8.decode(z))
