"""Image front and back end on the HIP path: every case of tests/golden/g12_frames.npz (the reference's load_img_and_K /
transform_img_and_K / save_output, oracle/make_goldens_frames.py) through the C-ABI, BIT FOR BIT -- the expression is fixed
(include/seva_hip.h) and its torch restatement (tests/fake_frame_ops.py) already equals the reference on the CPU, so there
is no tolerance: a differing bit is an FMA or a fast division in the kernel.  Then the contracts the other kernel families
hold (batch invariance, pitches, nothing written outside the output) and one end-to-end `pipeline.run_scene`."""
import pytest
import torch

from test_frames_cpu import f32_source, gold, run_case  # noqa: F401  (gold: fixture)

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from seva import _native
    _native.load()
    return torch.device("cuda:0")


def test_every_golden_case_bit_for_bit(dev, gold):
    g, cases = gold
    bad = []
    for c in cases:
        img, K = run_case(g, c, device=dev)
        want = g[c["id"] + "_img"]
        assert img.is_cuda and img.shape == want.shape and img.dtype == torch.float32, c["id"]
        diff = (img.cpu() != want)
        print(f"{c['id']}: {int(diff.sum())} of {want.numel()} values differ")
        if diff.any() or not torch.equal(K, g[c["id"] + "_K"]):
            bad.append((c["id"], int(diff.sum()), float((img.cpu() - want).abs().max())))
    assert not bad, bad


def _crop(src, out, **kw):
    from seva import ops
    ops.image_area_crop(src, out, **kw)
    torch.cuda.synchronize()
    return out


def _sources(dev, g):
    u4 = g["src_s1"].to(dev)                                   # (37, 53, 4)
    u3 = g["src_s2"].to(dev)                                   # (64, 48, 3)
    f = f32_source(g["src_t1"]).to(dev)[0]                     # (3, 37, 53)
    kw_u8 = dict(rh=12, rw=16, ct=-2, cl=-4, pad_value=1.0, out_mul=2.0, out_add=-1.0)  # load02's geometry: real padding
    kw_f = dict(rh=21, rw=30, ct=5, cl=6)                      # xform11's
    return [(u4, (16, 24), kw_u8), (u3, (20, 20), dict(rh=27, rw=20, ct=7, cl=0, out_mul=2.0, out_add=-1.0)), (f, (16, 24), kw_f)]


def test_result_of_an_image_does_not_depend_on_the_batch(dev, gold):
    g, _ = gold
    gen = torch.Generator().manual_seed(1)
    for x, (H, W), kw in _sources(dev, g):
        other = (torch.randint(0, 256, x.shape, generator=gen, dtype=torch.uint8) if x.dtype == torch.uint8
                 else torch.rand(x.shape, generator=gen) * 2 - 1).to(dev)
        one = _crop(x[None], torch.empty(1, 3, H, W, device=dev), **kw)
        three = _crop(torch.stack([other, x, other]), torch.empty(3, 3, H, W, device=dev), **kw)
        assert torch.equal(three[1], one[0]) and torch.equal(three[0], three[2]) and not torch.equal(three[0], three[1])


def test_pitches_and_guard_region(dev, gold):
    """Padded source rows / planes / images and a padded output image pitch give the dense result; the floats around and between
    the output images keep their sentinel."""
    g, _ = gold
    gen = torch.Generator().manual_seed(2)
    for x, (H, W), kw in _sources(dev, g):
        xs = torch.stack([x, x.flip(-2)])
        dense = _crop(xs, torch.empty(2, 3, H, W, device=dev), **kw)
        if x.dtype == torch.uint8:
            h, w, c = x.shape
            row = (w * c + 11) // 4 * 4 + 4 * (c == 4)         # RGBA pitches stay multiples of 4; RGB: 144 + 8 = 152 -> odd pixels
            row += 1 if c == 3 else 0
            pn = h * row + (8 if c == 4 else 7)
            buf = torch.randint(0, 256, (2 * pn + 16,), generator=gen, dtype=torch.uint8).to(dev)
            src = buf.as_strided((2, h, w, c), (pn, row, c, 1), 4)
        else:
            _, h, w = x.shape
            row, pc = w + 3, h * (w + 3) + 5
            pn = 3 * pc + 2
            buf = (torch.rand(2 * pn + 9, generator=gen) * 2 - 1).to(dev)
            src = buf.as_strided((2, 3, h, w), (pn, pc, row, 1), 3)
        src.copy_(xs)
        pitch, guard = 3 * H * W + 37, 129
        obuf = torch.full((2 * pitch + 2 * guard,), SENTINEL, device=dev)
        out = obuf.as_strided((2, 3, H, W), (pitch, H * W, W, 1), guard)
        _crop(src, out, **kw)
        assert torch.equal(out, dense), x.dtype
        out.fill_(SENTINEL)
        assert bool((obuf == SENTINEL).all())


def test_rgb_source_equals_opaque_rgba_source(dev, gold):
    g, _ = gold
    rgb = g["src_s2"].to(dev)[None]
    rgba = torch.cat([rgb, torch.full_like(rgb[..., :1], 255)], -1).contiguous()
    kw = dict(rh=43, rw=32, ct=13, cl=8, out_mul=2.0, out_add=-1.0)  # load07's geometry
    a = _crop(rgb, torch.empty(1, 3, 16, 16, device=dev), **kw)
    b = _crop(rgba, torch.empty(1, 3, 16, 16, device=dev), **kw)
    assert torch.equal(a, b) and torch.equal(a.cpu(), g["load07_img"])


def _u8_rule(x):
    t = (x.permute(0, 2, 3, 1) + 1) / 2.0
    return (t * 255).clamp(0, 255).to(torch.uint8)


def test_rgb_to_u8_on_the_crafted_tensor(dev, gold):
    """Every k/255*2-1 with its two fp32 neighbours, values outside [-1, 1], +-inf; NaN -> 0 (excluded from the comparison)."""
    from seva import frames
    g, _ = gold
    x = g["u8_in"]
    got = frames.to_uint8(x.to(dev)).cpu()
    nan = torch.isnan(x).permute(0, 2, 3, 1)
    assert int(nan.sum()) == 1 and int(got[nan][0]) == 0
    for want in (g["u8_out"], _u8_rule(x)):
        assert torch.equal(got[~nan], want[~nan]), int((got != want).sum())
    inf = torch.isinf(x).permute(0, 2, 3, 1)
    assert sorted(got[inf].tolist()) == [0, 255]


def test_rgb_to_u8_odd_image_with_a_pitch_and_guard(dev):
    """5 x 7 images: a partial last pixel group, a second image that starts on an odd byte, an input image pitch, and
    sentinel bytes around the output."""
    from seva import ops
    gen = torch.Generator().manual_seed(3)
    n, H, W, pitch, guard = 3, 5, 7, 3 * 35 + 6, 5
    x = torch.rand(n, 3, H, W, generator=gen) * 2.4 - 1.2
    xbuf = torch.full((n * pitch + 4,), float("nan"), device=dev)
    xs = xbuf.as_strided((n, 3, H, W), (pitch, H * W, W, 1), 2)
    xs.copy_(x)
    obuf = torch.full((n * H * W * 3 + 2 * guard,), 77, dtype=torch.uint8, device=dev)
    out = obuf[guard:guard + n * H * W * 3].view(n, H, W, 3)
    ops.rgb_to_u8(xs, out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), _u8_rule(x))
    assert bool((obuf[:guard] == 77).all()) and bool((obuf[-guard:] == 77).all())
    dense = torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev)
    ops.rgb_to_u8(x.to(dev), dense)
    assert torch.equal(dense, out)


def test_run_scene_end_to_end(dev):
    """Two 50 x 70 uint8 pictures -> 128 x 128 frames through the tiny UNet and the narrow synthetic VAE, T = 4, 2 steps."""
    from test_model_gpu import _build, _vae
    from seva import frames, pipeline
    from seva import synthetic as synth
    from seva.model import SGMWrapper
    net, _ = _build("tiny", dev)
    ae, _ = _vae(dev, (64, 64, 128, 128))
    gen = torch.Generator().manual_seed(9)
    images = [torch.randint(0, 256, (50, 70, 3), generator=gen, dtype=torch.uint8),
              torch.randint(0, 256, (50, 70, 4), generator=gen, dtype=torch.uint8).numpy()]
    n, ids = 10, [0, 1]
    c2ws, Ks = synth.orbit_c2w(n), synth.default_K(n)
    tok = torch.randn(1024, generator=gen)
    tok = (tok / tok.norm()).to(dev)
    with torch.no_grad():
        res = pipeline.run_scene(SGMWrapper(net), ae, images, c2ws, Ks, ids, size=(128, 128), clip_token=tok, T=4, num_steps=2,
                                 device=dev)
        assert res["frames"].dtype == torch.uint8 and res["frames"].shape == (n, 128, 128, 3) and res["frames"].is_cuda
        assert torch.equal(res["frames"], frames.to_uint8(ae.decode(res["latents"])))
        x = [frames.load_img_and_K(img, (128, 128), K=Ks[fid], device=dev) for img, fid in zip(images, ids)]
        assert torch.equal(res["latents"][ids], ae.encode(torch.cat([a for a, _ in x])))
        assert torch.equal(res["Ks"], torch.stack([k for _, k in x]))
    assert torch.isfinite(res["latents"]).all() and int(res["frames"].max()) > int(res["frames"].min())
