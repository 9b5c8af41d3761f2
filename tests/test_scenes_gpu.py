"""Scene folders through the HIP path: `scenes.run`, `anchor_ids`, `postprocess` and a two-mode sweep on the tiny UNet and the narrow
synthetic VAE of test_frames_gpu.py::test_run_scene_end_to_end (T = 4, 2 steps, 64 x 64 frames; synthetic weights throughout)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLD

pytestmark = pytest.mark.gpu

SCENES = os.path.join(GOLD, "scenes")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from seva import _native
    _native.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models(dev):
    from test_model_gpu import _build, _vae
    net, _ = _build("tiny", dev)
    ae, _ = _vae(dev, (64, 64, 128, 128))
    tok = torch.randn(1024, generator=torch.Generator().manual_seed(9))
    return net, ae, (tok / tok.norm()).to(dev)


def _task(name, *a, **k):
    from seva import scenes
    return scenes.read_scene(os.path.join(SCENES, name)).task(*a, **k)


def test_run_equals_run_scene_on_the_same_arrays(dev, models):
    from seva import pipeline, scenes
    from seva.model import SGMWrapper
    net, ae, tok = models
    t = _task("a_top", "img2img", 3, 4)
    kw = dict(clip_token=tok, num_steps=2, device=dev)
    with torch.no_grad():
        res = scenes.run(SGMWrapper(net), ae, t, size=(64, 64), use_traj_prior=False, **kw)
        Ks_in = t.Ks((64, 64))
        Ks_in[t.input_ids] = t.Ks_px[t.input_ids]
        direct = pipeline.run_scene(SGMWrapper(net), ae, [t.image_paths[i] for i in t.input_ids], t.c2ws, Ks_in, t.input_ids,
                                    size=(64, 64), use_traj_prior=False, targets={i: t.image_paths[i] for i in t.target_ids},
                                    T=4, options=t.options, task="img2img", **{**scenes.DEMO_DEFAULTS, **kw})
    assert res["frames"].shape == (12, 64, 64, 3) and res["frames"].is_cuda
    assert torch.equal(res["frames"], direct["frames"]) and torch.equal(res["latents"], direct["latents"])
    assert res["metrics"]["frame_ids"] == t.target_ids == direct["metrics"]["frame_ids"]
    for k in ("sse", "psnr", "ssim"):
        assert torch.equal(res["metrics"][k], direct["metrics"][k]), k
    assert torch.isfinite(res["metrics"]["psnr"]).all()


def test_two_passes_with_the_tasks_anchors_and_none_is_todays_call(dev, models):
    from seva import pipeline, scenes
    from seva.model import SGMWrapper
    net, ae, tok = models
    t = _task("b_mixed", "img2trajvid", "2-far", 4)
    kw = dict(clip_token=tok, num_steps=2, device=dev)
    with torch.no_grad():
        res = scenes.run(SGMWrapper(net), ae, t, size=(64, 64), use_traj_prior=True, **kw)
        assert res["plan"].anchor_ids == sorted(set(t.anchor_ids)) and len(res["plan"].pass2) >= 1
        assert torch.isfinite(res["latents"]).all() and int(res["frames"].max()) > int(res["frames"].min())
        assert torch.isfinite(res["metrics"]["psnr"]).all() and torch.isfinite(res["metrics"]["ssim"]).all()
        assert res["metrics"]["frame_ids"] == [i for i in t.target_ids if t.image_paths[i] is not None]
        Ks = t.Ks((64, 64))
        lat = res["latents"][t.input_ids]
        args = dict(clip_token=tok, T=4, num_steps=2, device=dev)
        a = pipeline.run_trajectory(SGMWrapper(net), lat, t.c2ws, Ks, t.input_ids, **args)
        b = pipeline.run_trajectory(SGMWrapper(net), lat, t.c2ws, Ks, t.input_ids, anchor_ids=None, **args)
    assert a["plan"] == b["plan"] and torch.equal(a["latents"], b["latents"])


def test_postprocess_scores_resized_frames(dev, models):
    from seva import frames, metrics, scenes
    from seva.model import SGMWrapper
    net, ae, tok = models
    t = _task("a_top", "img2img", 3, 4)
    with torch.no_grad():
        res = scenes.run(SGMWrapper(net), ae, t, size=(64, 64), use_traj_prior=False, postprocess={"resize": 32}, clip_token=tok,
                         num_steps=2, device=dev)
        tids = t.target_ids
        got = frames.to_uint8(frames.transform_img_and_K(res["rgb"][tids], 32)[0])
        tgt = torch.cat([frames.load_img_and_K(t.image_paths[i], (64, 64), device=dev)[0] for i in tids])
        want = frames.to_uint8(frames.transform_img_and_K(tgt, 32)[0])
        m = metrics.compare(got, want)
    assert got.shape == (len(tids), 32, 32, 3) and res["frames"].shape == (12, 64, 64, 3)
    assert res["metrics"]["frame_ids"] == tids and res["postprocess"] == {"resize": 32}
    for k in ("sse", "psnr", "ssim"):
        assert torch.equal(res["metrics"][k], m[k]), k


def test_two_mode_sweep_writes_a_report_and_frames(dev, models, tmp_path):
    from PIL import Image
    from seva import evaluate, scenes
    net, ae, tok = models
    rep = evaluate.main(["--scenes", os.path.join(SCENES, "b_mixed"), "--task", "img2img", "--size", "64,64", "--T", "4",
                         "--num-steps", "2", "--modes", "f16,rescale@0.5", "--out", str(tmp_path), "--device", str(dev)],
                        net=net, ae=ae, conditioner=lambda x: tok[None].expand(x.shape[0], -1))
    with open(tmp_path / "report.json") as f:
        assert json.load(f) == json.loads(json.dumps(rep))
    assert [(r["scene"], r["mode"]) for r in rep["rows"]] == [("b_mixed", "f16"), ("b_mixed", "rescale@0.5")]
    base, other = rep["rows"]
    assert base["vs_baseline"] == {"psnr": float("inf"), "ssim": 1.0} and np.isfinite(other["vs_baseline"]["psnr"])
    assert np.isfinite(base["psnr"]) and np.isfinite(other["psnr"]) and rep["input_encodes"] == 1
    from seva import frames
    t = _task("b_mixed", "img2img", "2-far", 4)
    loaded = torch.cat([frames.to_uint8(frames.load_img_and_K(t.image_paths[i], (64, 64), device=dev)[0]) for i in t.input_ids]).cpu().numpy()
    samples = {}
    for mode in ("f16", "rescale@0.5"):
        back = scenes.read_scene(tmp_path / "b_mixed" / mode)
        assert np.array_equal(back.c2ws, t.c2ws.double().numpy()) and np.array_equal(back.Ks, t.Ks_pixels((64, 64)).double().numpy())
        pics = []
        for p in back.image_paths:
            with Image.open(p) as im:
                assert im.size == (64, 64) and im.mode == "RGB"
                pics.append(np.array(im))
        # the input pictures on disk are the pictures as loaded; the samples are pictures, not a constant
        assert np.array_equal(np.stack([pics[i] for i in t.input_ids]), loaded)
        samples[mode] = np.stack([pics[i] for i in t.target_ids])
        assert samples[mode].shape == (6, 64, 64, 3) and samples[mode].max() > samples[mode].min()
    # the two modes' frames on disk differ, by what the report says: PSNR of the bytes read back == vs_baseline
    a, b = samples["f16"].astype(np.int64), samples["rescale@0.5"].astype(np.int64)
    assert not np.array_equal(a, b)
    sse = ((a - b) ** 2).sum(axis=(1, 2, 3))
    with np.errstate(divide="ignore"):
        psnr = np.where(sse == 0, np.inf, 10.0 * np.log10(255.0 ** 2 * 3 * 64 * 64 / np.maximum(sse, 1)))
    assert abs(psnr.mean() - other["vs_baseline"]["psnr"]) < 1e-9  # (fp64 on both sides: a few ulps of ~40 dB)
