"""Scene folders (`seva.scenes`), anchors from outside (`pipeline.plan_trajectory(anchor_ids=)`) and the mode sweep (`seva.evaluate`)
without a GPU.

a. Reader, tasks and intrinsics against tests/golden/g16_scenes.json: what the reference's `ReconfusionParser`, `parse_task` and the
   loading loop of `run_one_scene` make of the three folders under tests/golden/scenes/ (tools/make_goldens_scenes.py).  Every
   comparison is exact: cameras are the same float64 products cast once, intrinsics go through the host rules g12 pins.
b. `anchor_ids`: None is today's plan; a list lands in the first pass; bad ids raise.
c. `write_results` -> `read_scene` returns the cameras that were sampled and the frames that were generated.
d. `evaluate.main` on the fake network, the toy VAE and the fake frame / metric operators of the other CPU tests.
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLD

SCENES = os.path.join(GOLD, "scenes")
with open(os.path.join(GOLD, "g16_scenes.json")) as _f:
    G16 = json.load(_f)
SIZES = {"64x64": (64, 64), "L64": 64, "96x64": (96, 64)}


def _case_id(c):
    opt = ",".join(f"{k}={v}" for k, v in c["options"].items())
    return f"{c['scene']}-{c['task']}-{c['num_inputs']}-T{c['T']}" + (f"-{opt}" if opt else "")


def _scene(name):
    from seva import scenes
    return scenes.read_scene(os.path.join(SCENES, name))


def _T(t):
    return tuple(t) if isinstance(t, list) else t


# ---------------------------------------------------------------------------------------------------------------- a. golden
@pytest.mark.parametrize("name", sorted(G16["scenes"]))
def test_read_scene_equals_the_reference_parser(name):
    g, sc = G16["scenes"][name], _scene(name)
    assert len(sc) == len(g["image_names"]) and sc.image_names == g["image_names"]
    assert sc.image_paths == [None if p is None else os.path.join(SCENES, name, p) for p in g["image_paths"]]
    assert sc.c2ws.dtype == np.float64 and sc.c2ws.shape == (len(sc), 4, 4)
    assert np.array_equal(sc.c2ws, np.array(g["camtoworlds"], dtype=np.float64))
    assert sc.Ks.dtype == np.float64 and np.array_equal(sc.Ks, np.array(g["Ks"], dtype=np.float64))
    assert [list(s) for s in sc.sizes] == g["imsizes"]
    assert list(sc.splits.items()) == [(k, v) for k, v in g["splits"]]  # keys: an int where all digits, else the string
    if g["bounds"] is None:
        assert sc.bounds is None
    else:
        assert np.array_equal(sc.bounds, np.array(g["bounds"]))
    for i, p in enumerate(sc.image_paths):
        assert (sc.picture_size(i) is None) == (p is None)


def test_fixtures_cover_what_the_issue_lists():
    a, b, c = (G16["scenes"][n] for n in ("a_top", "b_mixed", "c_semidense"))
    assert len(a["image_names"]) == 12 and [k for k, _ in a["splits"]] == [3, 6]
    with open(os.path.join(SCENES, "a_top", "transforms.json")) as f:
        assert "applied_transform" in json.load(f)
    assert b["image_names"].count(None) == 1 and [k for k, _ in b["splits"]] == ["2-far"]
    assert len({tuple(s) for s in b["imsizes"]}) == 2
    assert len(c["image_names"]) == 40 and len(c["splits"][0][1]["train_ids"]) == 12
    assert any(t["scene"] == "c_semidense" and t["T"] == [41, 21] and t["T_after"] == [41, 21] for t in G16["tasks"])
    for n in G16["scenes"]:
        for root, _, files in os.walk(os.path.join(SCENES, n)):
            for fn in files:
                if fn.endswith(".png"):
                    from PIL import Image
                    with Image.open(os.path.join(root, fn)) as im:
                        assert max(im.size) <= 48


@pytest.mark.parametrize("case", G16["tasks"], ids=_case_id)
def test_task_equals_parse_task_and_the_loaded_intrinsics(case):
    sc = _scene(case["scene"])
    t = sc.task(case["task"], case["num_inputs"], _T(case["T"]), case["options"] or None)
    root = os.path.join(SCENES, case["scene"])
    assert t.image_paths == [None if p is None else os.path.join(root, p) for p in case["image_paths"]]
    assert (t.num_inputs, t.num_targets) == (case["num_inputs_out"], case["num_targets"])
    assert t.input_ids == case["input_indices"] and all(isinstance(i, int) for i in t.input_ids)
    assert t.target_ids == [i for i in range(len(t.image_paths)) if i not in case["input_indices"]]
    assert [float(a) for a in t.anchor_indices] == case["anchor_indices"]
    assert t.anchor_ids == case["anchor_ids"]
    assert t.T == _T(case["T"]) or list(t.T) == case["T"]
    assert t.T_passes == case["T_after"]
    assert t.c2ws.dtype == torch.float32 and t.c2ws.shape[1:] == (4, 4)
    assert torch.equal(t.c2ws[:, :3].double(), torch.tensor(case["c2ws"], dtype=torch.float64))
    assert torch.equal(t.c2ws[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(len(t.c2ws), 4))
    assert t.Ks_px.dtype == torch.float32 and torch.equal(t.Ks_px.double(), torch.tensor(case["Ks"], dtype=torch.float64))
    for tag, size in SIZES.items():
        g = case["Ks_at"][tag]
        Ks = t.Ks(size)
        assert Ks.dtype == torch.float32
        assert torch.equal(Ks.double(), torch.tensor(g["Ks"], dtype=torch.float64)), tag
        hw = {tuple(v) for v in g["frame_hw"]}
        if len(hw) == 1:
            assert t.frame_size(size) == tuple(reversed(next(iter(hw))))
            H, W = g["frame_hw"][0]  # `Ks_pixels`: the same intrinsics before the division by the frame's size
            assert torch.equal(t.Ks_pixels(size)[:, 0] / W, Ks[:, 0]) and torch.equal(t.Ks_pixels(size)[:, 1] / H, Ks[:, 1])
        else:  # L_short on pictures of both orientations: the reference's loop ends with frames it cannot stack
            assert tag == "L64" and case["scene"] == "b_mixed"
            from seva import scenes
            with pytest.raises(scenes.SceneError, match="different sizes"):
                t.frame_size(size)


def test_a_frame_without_a_picture_takes_the_size_of_the_last_one_that_had_one():
    t = _scene("b_mixed").task("img2trajvid", "2-far", 6)
    j = t.image_paths.index(None)
    sizes = t.picture_sizes()
    assert j > 0 and sizes[j] == sizes[j - 1] and tuple(t.scene.sizes[t.scene_ids[j]]) != sizes[j]
    assert _scene("b_mixed").task("img2img", None, 21).num_inputs == 2  # the only split, a string key: "2-far" means 2 inputs


def test_errors_name_the_file_and_the_key(tmp_path):
    import shutil
    from seva import scenes
    with pytest.raises(scenes.SceneError, match=r"train_test_split_\*\.json.*2 splits"):
        _scene("a_top").task("img2img", None)
    with pytest.raises(scenes.SceneError, match="no split 4"):
        _scene("a_top").task("img2img", 4)
    with pytest.raises(scenes.SceneError, match="unknown task"):
        _scene("a_top").task("img2trajvid_s-prob", 3)
    d = tmp_path / "nosplit"
    shutil.copytree(os.path.join(SCENES, "a_top"), d)
    for k in (3, 6):
        os.remove(d / f"train_test_split_{k}.json")
    with pytest.raises(scenes.SceneError, match="no split"):
        scenes.read_scene(d).task("img2img", 3)
    with open(d / "transforms.json") as f:
        meta = json.load(f)
    for key, where in (("fl_y", "top"), ("transform_matrix", "frame"), ("frames", "top")):
        bad = json.loads(json.dumps(meta))
        if where == "top":
            del bad[key]
        else:
            del bad["frames"][2][key]
        with open(d / "transforms.json", "w") as f:
            json.dump(bad, f)
        with pytest.raises(scenes.SceneError, match=rf"transforms\.json.*'{key}'"):
            scenes.read_scene(d)
    with pytest.raises(scenes.SceneError, match="no such file"):
        scenes.read_scene(tmp_path / "absent")
    # img2img is one pass only: asked for two, it fails before anything is loaded or run
    t = _scene("a_top").task("img2img", 3)
    with pytest.raises(scenes.SceneError, match="one pass only"):
        scenes.run(None, None, t, size=(64, 64), use_traj_prior=True)
    with pytest.raises(ValueError, match="postprocess"):
        scenes.run(None, None, t, size=(64, 64), use_traj_prior=False, postprocess={"blur": 3})


# -------------------------------------------------------------------------------------------------------------- b. anchor_ids
def _golden_trajectories():
    from seva import synthetic as synth
    with open(os.path.join(GOLD, "g10_two_pass_plans.json")) as f:
        g10 = json.load(f)
    z = np.load(os.path.join(GOLD, "g10_two_pass_cams.npz"))
    for name, g in g10.items():
        yield name, torch.from_numpy(z[name]), g, {}
    with open(os.path.join(GOLD, "g15_semidense_plans.json")) as f:
        g15 = json.load(f)
    for name, g in g15.items():
        yield name, synth.orbit_c2w(g["n"]), g, {"options": g["options"] or None}


def test_anchor_ids_none_is_todays_plan():
    from seva import pipeline
    seen = 0
    for name, c2ws, g, kw in _golden_trajectories():
        args = dict(T=_T(g["T"]), chunk_strategy=g["chunk_strategy"], first_pass_strategy=g["first_pass_strategy"], **kw)
        today = pipeline.plan_trajectory(c2ws, g["input_ids"], **args)
        assert pipeline.plan_trajectory(c2ws, g["input_ids"], anchor_ids=None, **args) == today, name
        assert today.anchor_ids == g["prior_inds"], name
        # the planner's own choice handed back from outside: the same plan again
        assert pipeline.plan_trajectory(c2ws, g["input_ids"], anchor_ids=list(reversed(today.anchor_ids)), **args) == today, name
        seen += 1
    assert seen >= 10


def test_given_anchor_ids_are_the_first_pass():
    from seva import pipeline
    t = _scene("a_top").task("img2trajvid", 3, 6, {"chunk_strategy": "interp"})
    assert t.anchor_ids == [3, 6, 8, 11]  # round, where the planner's own rule takes the ceiling
    args = dict(T=6, chunk_strategy="interp", options=t.options)
    own = pipeline.plan_trajectory(t.c2ws, t.input_ids, **args)
    plan = pipeline.plan_trajectory(t.c2ws, t.input_ids, anchor_ids=t.anchor_ids, **args)
    assert own.anchor_ids == [3, 6, 9, 11] and plan.anchor_ids == t.anchor_ids
    assert sorted(f for w in plan.pass1 for f in w.target_ids) == t.anchor_ids
    assert {f for w in plan.pass2 for f in w.source_ids} <= set(t.input_ids + t.anchor_ids)
    assert sorted({f for w in plan.pass2 for f in w.target_ids}) == t.target_ids
    assert (plan.T1, plan.T2) == (own.T1, own.T2)
    # an id the rounding rule repeats counts once
    assert pipeline.plan_trajectory(t.c2ws, t.input_ids, anchor_ids=t.anchor_ids + [6], **args) == plan
    for bad, msg in (([3, 12], "outside"), ([-1], "outside"), ([0, 5], "input views"), ([], "empty"), ([3.5], "integer")):
        with pytest.raises(ValueError, match=msg):
            pipeline.plan_trajectory(t.c2ws, t.input_ids, anchor_ids=bad, **args)


# ------------------------------------------------------------------------------------------------------ c., d. on fake operators
@pytest.fixture
def cpu(monkeypatch):
    import fake_frame_ops
    import fake_metric_ops
    import seva.ops as ops
    from test_pipeline_cpu import _patch_cpu
    _patch_cpu(monkeypatch)
    monkeypatch.setattr(ops, "frame_metrics", fake_metric_ops.frame_metrics)
    monkeypatch.setattr(ops, "image_area_crop", fake_frame_ops.image_area_crop)
    monkeypatch.setattr(ops, "rgb_to_u8", fake_frame_ops.rgb_to_u8)


def _token():
    tok = torch.randn(1024, generator=torch.Generator().manual_seed(5))
    return tok / tok.norm()


def test_run_is_run_scene_on_the_tasks_arrays(cpu):
    from test_frames_cpu import _ToyAE
    from test_pipeline_cpu import _fake_net
    from seva import pipeline, scenes
    t = _scene("a_top").task("img2img", 3, 4)
    kw = dict(clip_token=_token(), num_steps=2, device="cpu")
    res = scenes.run(_fake_net, _ToyAE(), t, size=(64, 64), use_traj_prior=False, **kw)
    Ks = t.Ks((64, 64))
    Ks_in = Ks.clone()
    Ks_in[t.input_ids] = t.Ks_px[t.input_ids]
    direct = pipeline.run_scene(_fake_net, _ToyAE(), [t.image_paths[i] for i in t.input_ids], t.c2ws, Ks_in, t.input_ids,
                                size=(64, 64), use_traj_prior=False, targets={i: t.image_paths[i] for i in t.target_ids},
                                T=4, options=t.options, task="img2img", **{**scenes.DEMO_DEFAULTS, **kw})
    assert torch.equal(res["frames"], direct["frames"]) and torch.equal(res["latents"], direct["latents"])
    assert res["metrics"]["frame_ids"] == t.target_ids
    for k in ("sse", "psnr", "ssim"):
        assert torch.equal(res["metrics"][k], direct["metrics"][k])
    # what was sampled for the input views is the task's Ks, bit for bit
    assert torch.equal(direct["Ks"] / direct["Ks"].new_tensor([64, 64, 1.0])[:, None], Ks[t.input_ids])



def test_run_plans_under_the_tasks_chunk_strategy(cpu):
    """The strategy a task is stated under (its anchors and window lengths follow it) is the one the windows are planned under."""
    from test_frames_cpu import _ToyAE
    from test_pipeline_cpu import _fake_net
    from seva import pipeline, scenes
    t = _scene("a_top").task("img2trajvid", 3, 6, {"chunk_strategy": "interp"})
    kw = dict(clip_token=_token(), num_steps=2, device="cpu")
    res = scenes.run(_fake_net, _ToyAE(), t, size=(64, 64), use_traj_prior=True, **kw)
    want = pipeline.plan_trajectory(t.c2ws, t.input_ids, T=6, chunk_strategy="interp", options=t.options, anchor_ids=t.anchor_ids)
    assert res["plan"] == want and len(want.pass2) == 3
    assert res["plan"] != pipeline.plan_trajectory(t.c2ws, t.input_ids, T=6, chunk_strategy="nearest-gt", anchor_ids=t.anchor_ids)
    same = scenes.run(_fake_net, _ToyAE(), t, size=(64, 64), use_traj_prior=True, chunk_strategy="interp", **kw)
    assert same["plan"] == want and torch.equal(same["frames"], res["frames"])
    for bad in (dict(chunk_strategy="nearest-gt"), dict(options={"chunk_strategy": "gt"})):
        with pytest.raises(scenes.SceneError, match="stated under 'interp'"):
            scenes.run(_fake_net, _ToyAE(), t, size=(64, 64), use_traj_prior=True, **bad, **kw)
    # semi-dense: the plan's window lengths are the task's
    t = _scene("c_semidense").task("img2trajvid", 12, 21, {"chunk_strategy": "interp-gt"})
    res = scenes.run(_fake_net, _ToyAE(), t, size=(64, 64), use_traj_prior=True, **kw)
    assert [res["plan"].T1, res["plan"].T2] == t.T_passes == [21, 33] and res["plan"].anchor_ids == t.anchor_ids
    # one pass: `plan_views` under the task's strategy too
    t = _scene("a_top").task("img2vid", 3, 8, {"chunk_strategy": "interp"})
    res = scenes.run(_fake_net, _ToyAE(), t, size=(64, 64), use_traj_prior=False, **kw)
    assert res["plan"] == pipeline.plan_views(t.c2ws, t.input_ids, 8, "interp", t.options, "img2vid")


def test_write_results_then_read_scene_round_trip(cpu, tmp_path):
    from PIL import Image
    from test_frames_cpu import _ToyAE
    from test_pipeline_cpu import _fake_net
    from seva import scenes
    t = _scene("b_mixed").task("img2trajvid", "2-far", 4)
    assert None in t.image_paths
    res = scenes.run(_fake_net, _ToyAE(), t, size=(64, 64), use_traj_prior=True, clip_token=_token(), num_steps=2, device="cpu")
    assert res["plan"].anchor_ids == sorted(set(t.anchor_ids)) and res["frames"].shape == (8, 64, 64, 3)
    assert res["metrics"]["frame_ids"] == [i for i in t.target_ids if t.image_paths[i] is not None]
    rec = scenes.write_results(tmp_path / "out", res, t, options={"num_steps": 2})
    with open(tmp_path / "out" / "train_test_split_5.json", "w") as f:  # left by an earlier result in the same folder
        json.dump({"train_ids": [0], "test_ids": [1]}, f)
    rec = scenes.write_results(tmp_path / "out", res, t, options={"num_steps": 2})
    back = scenes.read_scene(tmp_path / "out")
    assert list(back.splits) == [2]
    assert np.array_equal(back.c2ws, t.c2ws.double().numpy())
    assert np.array_equal(back.Ks, t.Ks_pixels((64, 64)).double().numpy())
    assert all(tuple(s) == (64, 64) for s in back.sizes)
    # read again as a task at the frames' own size: the intrinsics that were sampled, bit for bit
    t2 = back.task("img2trajvid", None, 4)
    assert t2.input_ids == t.input_ids and t2.target_ids == t.target_ids and t2.anchor_ids == t.anchor_ids
    assert torch.equal(t2.c2ws, t.c2ws) and torch.equal(t2.Ks((64, 64)), t.Ks((64, 64)))
    # the PNG bytes are the frames
    for j, fid in enumerate(t.target_ids):
        assert back.image_paths[fid] == os.path.join(str(tmp_path / "out"), "./samples-rgb", f"{j:03d}.png")
        with Image.open(back.image_paths[fid]) as im:
            assert im.mode == "RGB" and np.array_equal(np.array(im), res["frames"][fid].numpy())
    for j, fid in enumerate(t.input_ids):
        with Image.open(back.image_paths[fid]) as im:
            assert np.array_equal(np.array(im), res["input_frames"][j].numpy())
    with open(tmp_path / "out" / "metrics.json") as f:
        m = json.load(f)
    assert m == json.loads(json.dumps(rec)) and m["frame_ids"] == res["metrics"]["frame_ids"] and m["options"] == {"num_steps": 2}
    assert m["psnr"] == [float(v) for v in res["metrics"]["psnr"]] and m["mean"]["ssim"] == pytest.approx(float(res["metrics"]["ssim"].mean()), abs=1e-15)
    assert "lpips" not in m and m["anchor_ids"] == t.anchor_ids


def _fake_clip(x):
    return x.mean((2, 3)).repeat(1, 342)[:, :1024]


def test_evaluate_sweeps_modes_over_scenes(cpu, tmp_path, capsys):
    from test_frames_cpu import _ToyAE
    from test_pipeline_cpu import _fake_net
    from seva import evaluate
    calls = []

    def net(x, t, cond, num_frames):
        calls.append(x.shape[0])
        return _fake_net(x, t, cond, num_frames)

    dirs = ",".join(os.path.join(SCENES, n) for n in ("a_top", "c_semidense"))
    argv = ["--scenes", dirs, "--task", "img2img", "--size", "64,64", "--T", "16", "--num-steps", "2",
            "--modes", "f16,cache@2", "--out", str(tmp_path / "sweep"), "--device", "cpu"]
    with pytest.raises(ValueError, match="unknown mode token 'int4'"):
        evaluate.main([*argv[:-6], "--modes", "f16,int4", *argv[-4:]], net=net, ae=_ToyAE(), conditioner=_fake_clip)
    assert not calls and not os.path.exists(tmp_path / "sweep")  # before any work
    from seva import scenes
    with pytest.raises(scenes.SceneError, match="2 splits"):  # a_top has two: the split has to be named
        evaluate.main(argv, net=net, ae=_ToyAE(), conditioner=_fake_clip)
    assert not calls
    dirs = ",".join(os.path.join(SCENES, n) for n in ("b_mixed", "c_semidense"))
    argv[1] = dirs
    rep = evaluate.main(argv, net=net, ae=_ToyAE(), conditioner=_fake_clip)
    assert calls
    assert [(r["scene"], r["mode"]) for r in rep["rows"]] == [("b_mixed", "f16"), ("b_mixed", "cache@2"), ("c_semidense", "f16"),
                                                               ("c_semidense", "cache@2")]
    assert rep["input_encodes"] == 2  # input latents: once per scene, not once per mode
    for r in rep["rows"]:
        assert np.isfinite(r["psnr"]) and 0 < r["ssim"] < 1 and r["frames"] in (6, 28)
        if r["mode"] == "f16":
            assert r["vs_baseline"]["psnr"] == float("inf") and r["vs_baseline"]["ssim"] == 1.0
    assert [m["mode"] for m in rep["means"]] == ["f16", "cache@2"] and all(m["scenes"] == 2 for m in rep["means"])
    with open(tmp_path / "sweep" / "report.json") as f:
        assert json.load(f) == json.loads(json.dumps(rep))
    out = capsys.readouterr().out
    assert "cache@2" in out and "(mean)" in out and "inf" in out
    back = scenes.read_scene(tmp_path / "sweep" / "c_semidense" / "cache@2")
    assert len(back) == 40 and os.path.exists(tmp_path / "sweep" / "b_mixed" / "f16" / "metrics.json")


def test_mode_registry():
    from seva import evaluate as E
    assert E.split_modes("f16,interval@0.5,20,rescale@0.7+cache@3") == ["f16", "interval@0.5,20", "rescale@0.7+cache@3"]
    assert E.split_modes("interval@0.5,inf+fp8,fp8+attn") == ["interval@0.5,inf+fp8", "fp8+attn"]
    names = [s["name"] for s in E.parse_modes("fp8,vae-fp8")]
    assert names == ["f16", "fp8", "vae-fp8"]  # the baseline always runs, first
    for name in ("f16", "fp8", "fp8+attn", "fp8+ff", "split-all", "vae-fp8", "vae-phases", "dpmpp2m@20", "cache@2", "interval@0.5,20",
                 "rescale@0.7"):
        E.parse_mode(name)
    assert E.parse_mode("fp8+attn+ff")["net"] == {"precision": "fp8", "attention": "fp8", "ff": "fp8"}
    assert E.parse_mode("dpmpp2m@20+vae-phases") == {"name": "dpmpp2m@20+vae-phases", "net": {}, "vae": {"upsample": "phases"},
                                                     "run": {"solver": "dpmpp2m", "num_steps": 20}}
    assert E.parse_mode("interval@0.5,inf+rescale@0.7+cache@3/2")["run"] == {
        "guidance_interval": (0.5, float("inf")), "guidance_rescale": 0.7, "cache_interval": 3, "cache_levels": 2}
    for bad in ("attn", "f16+ff", "fp8+split-all", "f16+fp8", "cache", "cache@x", "fp8@3", "interval@3", "fp8+fp8", "bf16"):
        with pytest.raises(ValueError):
            E.parse_mode(bad)

    class Net:
        def set_precision(self, precision, **kw):
            self.got = (precision, kw)

    class Vae:
        def set_precision(self, p):
            self.p = p

        def set_upsample(self, u):
            self.u = u

    net, vae = Net(), Vae()
    E.apply_mode(E.parse_mode("fp8+attn+vae-phases"), net, vae)
    assert net.got == ("fp8", {"attention": "fp8", "ff": None, "split": None}) and (vae.p, vae.u) == ("f16", "phases")
    E.apply_mode(E.parse_mode("f16"), net, vae)  # a mode never inherits the one before it
    assert net.got == ("f16", {"attention": None, "ff": None, "split": None}) and (vae.p, vae.u) == ("f16", "taps")
    with pytest.raises(ValueError, match="no set_precision"):
        E.apply_mode(E.parse_mode("fp8"), lambda *a: None, vae)


def test_missing_weights_are_named(cpu, tmp_path, monkeypatch):
    from test_frames_cpu import _ToyAE
    from test_pipeline_cpu import _fake_net
    from seva import evaluate
    for v in evaluate.WEIGHTS.values():
        monkeypatch.delenv(v, raising=False)
    argv = ["--scenes", os.path.join(SCENES, "b_mixed"), "--size", "64,64", "--T", "4", "--out", str(tmp_path / "o"), "--device", "cpu"]
    with pytest.raises(SystemExit, match="--model"):
        evaluate.main(argv, ae=_ToyAE(), conditioner=_fake_clip)
    with pytest.raises(SystemExit, match="SEVA_VAE_PATH"):
        evaluate.main(argv, net=_fake_net, conditioner=_fake_clip)
    with pytest.raises(SystemExit, match="SEVA_CLIP_PATH"):
        evaluate.main(argv, net=_fake_net, ae=_ToyAE())
    with pytest.raises(SystemExit, match="no such file"):
        evaluate.main([*argv, "--clip", str(tmp_path / "absent.safetensors")], net=_fake_net, ae=_ToyAE())
