"""Image front and back end (`seva.frames`, `pipeline.run_scene`) without a GPU: the host geometry and intrinsics against
every case of tests/golden/g12_frames.npz (generated from the reference by oracle/make_goldens_frames.py), and the
arithmetic contract of the two kernels -- restated in torch in tests/fake_frame_ops.py -- against the reference's images
bit for bit.  tests/test_frames_gpu.py holds the same comparisons for the HIP kernels."""
import json
import os

import pytest
import torch

from conftest import ROOT, load_golden


@pytest.fixture(scope="module")
def gold():
    g = load_golden("g12_frames")
    return g, json.loads(str(g["cases"]))


def f32_source(u8: torch.Tensor) -> torch.Tensor:
    """The float sources of the transform cases, as the generator derives them from the stored bytes."""
    return (u8.permute(0, 3, 1, 2).contiguous().float() / 255.0) * 2.0 - 1.0


def run_case(g, c, device="cpu", png_dir=None):
    """One golden case through seva.frames -> (image, K)."""
    from seva import frames
    kw = dict(scale=c["scale"], center=tuple(c["center"]), size_stride=c["size_stride"], K=g[c["id"] + "_Kin"])
    size = tuple(c["size"]) if isinstance(c["size"], list) else c["size"]
    if c["kind"] == "transform":
        return frames.transform_img_and_K(f32_source(g["src_" + c["src"]]).to(device), size, mode=c["mode"], **kw)
    src = g["src_" + c["src"]]
    if c["blank"]:
        src = torch.Size((c["h"], c["w"]))
    elif png_dir is not None:
        from PIL import Image
        path = os.path.join(png_dir, c["id"] + ".png")
        Image.fromarray(src.numpy()).save(path)
        src = path
    return frames.load_img_and_K(src, size, center_crop=c["center_crop"], context_rgb=g["ctx_" + c["src"]] if c["ctx"] else None,
                                 device=device, **kw)


@pytest.fixture
def fake(monkeypatch):
    import fake_frame_ops
    import seva.ops as ops
    monkeypatch.setattr(ops, "image_area_crop", fake_frame_ops.image_area_crop)
    monkeypatch.setattr(ops, "rgb_to_u8", fake_frame_ops.rgb_to_u8)


def test_factor_and_shortest_side_equal_the_reference(gold):
    from seva import frames
    g, _ = gold
    for (th, tw, ch, cw, cover), want in zip(g["factor_args"].tolist(), g["factor"].tolist()):
        assert frames.get_resizing_factor((th, tw), (ch, cw), bool(cover)) == want, (th, tw, ch, cw, cover)
    for (w, h, s), want in zip(g["wh_args"].tolist(), g["wh"].tolist()):
        assert list(frames.get_wh_with_fixed_shortest_side(w, h, None if s < 0 else s)) == want


def test_plans_and_intrinsics_equal_every_golden_case(gold):
    from seva import frames
    g, cases = gold
    assert len(cases) >= 30
    for c in cases:
        size = tuple(c["size"]) if isinstance(c["size"], list) else c["size"]
        if c["kind"] == "load":
            p = frames.plan_load(c["h"], c["w"], size, c["scale"], c["center"], c["size_stride"], c["center_crop"])
            K = frames.adjust_K(g[c["id"] + "_Kin"], p, c["h"], c["w"], shift=(-p.cl, -p.ct))
        else:
            p = frames.plan_transform(c["h"], c["w"], size, c["scale"], c["center"], c["size_stride"], c["mode"])
            K = frames.adjust_K(g[c["id"] + "_Kin"], p, c["h"], c["w"])
        assert list(p) == c["plan"] and all(isinstance(v, int) for v in p), (c["id"], tuple(p), c["plan"])
        assert K.dtype == torch.float32 and torch.equal(K, g[c["id"] + "_K"]), c["id"]


def test_stated_arithmetic_reproduces_every_golden_image(gold, fake):
    g, cases = gold
    for c in cases:
        img, K = run_case(g, c)
        want = g[c["id"] + "_img"]
        assert img.shape == want.shape and img.dtype == torch.float32, c["id"]
        assert torch.equal(img, want), (c["id"], float((img - want).abs().max()))
        assert torch.equal(K, g[c["id"] + "_K"]), c["id"]


def test_png_path_and_rgb_source(gold, fake, tmp_path):
    """A PNG read through PIL gives what its bytes give; a 3-channel array what the opaque 4-channel one gives."""
    from seva import frames
    g, cases = gold
    for c in [c for c in cases if c["kind"] == "load" and not c["blank"]][:4] + [c for c in cases if c["src"] == "s2"][:1]:
        img, _ = run_case(g, c, png_dir=str(tmp_path))
        assert torch.equal(img, g[c["id"] + "_img"]), c["id"]
    rgb = g["src_s2"]
    rgba = torch.cat([rgb, torch.full_like(rgb[..., :1], 255)], -1)
    a, _ = frames.load_img_and_K(rgb.numpy(), (20, 20), device="cpu")
    b, _ = frames.load_img_and_K(rgba, (20, 20), device="cpu")
    assert torch.equal(a, b)


def test_uint8_rule_equals_save_output(gold, fake):
    from seva import frames
    g, _ = gold
    x, want = g["u8_in"], g["u8_out"]
    got = frames.to_uint8(x)
    nan = torch.isnan(x).permute(0, 2, 3, 1)
    assert int(nan.sum()) == 1 and got.dtype == torch.uint8 and got.shape == want.shape
    assert torch.equal(got[~nan], want[~nan]) and int(got[nan].max()) == 0
    assert int(want.min()) == 0 and int(want.max()) == 255


def test_arguments_are_checked_and_there_is_no_cpu_fallback():
    from seva import _native, frames
    with pytest.raises(ValueError):
        frames.load_img_and_K(torch.Size((8, 8)), None, image_as_tensor=False, device="cpu")
    with pytest.raises(ValueError):
        frames.plan_transform(8, 8, (4, 4), mode="fit")
    with pytest.raises(ValueError):
        frames.load_img_and_K(torch.zeros(8, 8, 3), None, device="cpu")  # not uint8
    with pytest.raises(_native.SevaNativeError):
        frames.load_img_and_K(torch.zeros(8, 8, 3, dtype=torch.uint8), None, device="cpu")
    with pytest.raises(_native.SevaNativeError):
        frames.to_uint8(torch.zeros(1, 3, 4, 4))
    assert not os.path.exists(os.path.join(ROOT, "stable-virtual-camera_amd", "seva", "eval.py"))  # would shadow the reference's


class _ToyAE:
    """encode: 8x8 block means of the three channels + their mean; decode: nearest upsampling of three mixes."""

    def encode(self, x):
        z = torch.nn.functional.avg_pool2d(x, 8)
        return torch.cat([z, z.mean(1, keepdim=True)], 1) * 0.5

    def decode(self, z):
        rgb = torch.stack([z[:, 0] + z[:, 3], z[:, 1] - z[:, 3], z[:, 2] * 1.5], 1)
        return torch.nn.functional.interpolate(rgb, scale_factor=8, mode="nearest")


def test_run_scene_is_the_composition_of_its_parts(gold, fake, monkeypatch):
    from test_pipeline_cpu import _fake_net, _patch_cpu
    from seva import frames, pipeline
    from seva import synthetic as synth
    _patch_cpu(monkeypatch)
    g, _ = gold
    n, ids = 12, [0, 1]
    images = [g["src_s1"].numpy(), g["src_s2"]]  # an RGBA array and an RGB tensor
    c2ws, Ks = synth.orbit_c2w(n), synth.default_K(n)
    tok = torch.randn(1024, generator=torch.Generator().manual_seed(5))
    ae = _ToyAE()
    res = pipeline.run_scene(_fake_net, ae, images, c2ws, Ks, ids, size=(48, 32), clip_token=tok / tok.norm(), T=4, num_steps=2,
                             device="cpu")
    assert res["frames"].dtype == torch.uint8 and res["frames"].shape == (n, 32, 48, 3)
    assert torch.equal(res["frames"], frames.to_uint8(ae.decode(res["latents"])))
    assert torch.equal(res["rgb"], ae.decode(res["latents"]))
    for i, fid in enumerate(ids):
        x, K = frames.load_img_and_K(images[i], (48, 32), K=Ks[fid], device="cpu")
        assert torch.equal(res["latents"][fid], ae.encode(x)[0])
        assert torch.equal(res["Ks"][i], K)
    assert float(res["latents"][1].abs().max()) > 0
