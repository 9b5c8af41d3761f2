"""Scores of generated frames (`seva.metrics`) and the one-pass view driver (`pipeline.plan_views` / `run_views` /
`run_scene(use_traj_prior=False, targets=...)`) without a GPU.  `ops.frame_metrics` is replaced by tests/fake_metric_ops.py, a
plain-torch fp32 restatement of the contract in include/seva_hip.h: what is under test is the contract against an fp64 SSIM,
the host arithmetic (MSE, PSNR, normalisation), the argument checks and the orchestration.  tests/test_metrics_gpu.py holds
the same comparisons for the HIP kernels."""
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import metric_cases as MC
from conftest import ROOT


@pytest.fixture
def fake(monkeypatch):
    import fake_frame_ops
    import fake_metric_ops
    import seva.ops as ops
    monkeypatch.setattr(ops, "frame_metrics", fake_metric_ops.frame_metrics)
    monkeypatch.setattr(ops, "image_area_crop", fake_frame_ops.image_area_crop)
    monkeypatch.setattr(ops, "rgb_to_u8", fake_frame_ops.rgb_to_u8)


@pytest.mark.parametrize("case", [c[0] for c in MC.all_cases()])
def test_compare_against_fp64(case, fake):
    from seva import metrics
    a, b = next((a, b) for cid, a, b in MC.all_cases() if cid == case)
    sse, ssim, smap = MC.reference(case)
    n, H, W, _ = a.shape
    for kind, (xa, xb) in {"u8": (a, b), "f32": (MC.to_f32(a), MC.to_f32(b))}.items():
        m = metrics.compare(xa, xb, ssim_map=True)
        assert m["sse"].dtype == torch.int64 and torch.equal(m["sse"], sse), (case, kind)
        assert m["mse"].dtype == m["psnr"].dtype == m["ssim"].dtype == torch.float64
        assert torch.equal(m["mse"], sse.double() / (3 * H * W))
        e_frame, e_map = float((m["ssim"] - ssim).abs().max()), float((m["ssim_map"].double() - smap).abs().max())
        print(f"{case} {kind}: ssim {ssim.tolist()} frame err {e_frame:.3e} map err {e_map:.3e}")
        assert m["ssim_map"].shape == (n, 3, H - 10, W - 10) and m["ssim_map"].dtype == torch.float32
        assert e_frame < MC.FRAME_TOL and e_map < MC.MAP_TOL, (case, kind, e_frame, e_map)
    if case == "identical":
        assert torch.equal(m["ssim"], torch.ones(n, dtype=torch.float64)) and int(m["sse"].abs().max()) == 0


def test_psnr_formula_inf_and_wrappers(fake):
    from seva import metrics
    a, b = MC.pair("smooth_pm6")
    m = metrics.compare(a, b, ssim=False)
    assert set(m) == {"sse", "mse", "psnr"}
    want = 10.0 * torch.log10(255.0 ** 2 * (3 * MC.H0 * MC.W0) / MC.sse_i64(a, b).double())
    assert torch.allclose(m["psnr"], want, rtol=0, atol=1e-12) and 30 < float(want.min()) < 45
    assert torch.equal(metrics.psnr(a, b), m["psnr"])
    assert torch.equal(metrics.ssim(a, b), metrics.compare(a, b)["ssim"])
    same = metrics.compare(a, a.clone())
    assert torch.isinf(same["psnr"]).all() and (same["psnr"] > 0).all() and torch.equal(same["ssim"], torch.ones(3, dtype=torch.float64))
    w, k = MC.pair("white_black")
    assert torch.equal(metrics.psnr(w, k), torch.zeros(3, dtype=torch.float64))  # mse = 255^2
    mixed = metrics.psnr(torch.cat([a[:1], a[:1]]), torch.cat([a[:1], b[:1]]))  # inf and finite in one batch
    assert torch.isinf(mixed[0]) and mixed[1] == m["psnr"][0]
    small = metrics.compare(a[:, :5, :7], b[:, :5, :7], ssim=False)  # no size limit without SSIM
    assert torch.equal(small["sse"], MC.sse_i64(a[:, :5, :7], b[:, :5, :7]))


def test_arguments_are_checked_and_there_is_no_cpu_fallback(fake, monkeypatch):
    import seva.ops as ops
    from seva import _native, metrics
    a, b = MC.pair("noise")
    for bad in [(a, b[:2]), (a, b[:, :-1]), (a, MC.to_f32(b)), (a.float(), b.float()), (a[0], b[0]), (a[..., :2], b[..., :2]),
                (MC.to_f32(a).double(), MC.to_f32(b).double()), (a.numpy(), b.numpy())]:
        with pytest.raises(ValueError):
            metrics.compare(*bad)
    with pytest.raises(ValueError):
        metrics.compare(a, b, ssim=False, ssim_map=True)
    with pytest.raises(_native.SevaNativeError):  # H < 11 with SSIM: the library's error
        metrics.compare(a[:, :10], b[:, :10])
    monkeypatch.undo()  # the real operator: CPU tensors are refused, nothing is computed in torch
    assert ops.frame_metrics.__module__ == "seva.ops"
    for fn in (metrics.compare, metrics.psnr, metrics.ssim):
        with pytest.raises(_native.SevaNativeError):
            fn(a, b)


def test_new_symbols_in_header_and_binding():  # (header against binding: tests/test_abi_cpu.py)
    mk = open(os.path.join(ROOT, "stable-virtual-camera_amd", "csrc", "Makefile")).read()
    assert "metrics.hip" in re.search(r"^SRCS\s*:=\s*(.+)$", mk, re.M).group(1).split()


# ---- the one-pass driver -------------------------------------------------------------------------------------------------
def _scene(n=30, hw=8):
    from test_pipeline_cpu import _scene as scene
    return scene(n, hw)


@pytest.mark.parametrize("strategy", ["gt", "gt-nearest"])
def test_plan_views_generates_every_frame_once(strategy):
    from seva import pipeline
    n, ins, T = 50, [0, 25], 21
    c2ws, _, _, _ = _scene(n)
    plan = pipeline.plan_views(c2ws, ins, T=T, chunk_strategy=strategy)
    assert plan.pass2 == [] and plan.input_ids == ins and plan.pass1_serial == (strategy != "gt")
    gen = [f for w in plan.pass1 for f in w.target_ids]
    assert sorted(gen) == [f for f in range(n) if f not in ins] == sorted(plan.anchor_ids) and len(gen) == len(set(gen))
    assert len(plan.pass1) >= 3 and [w.global_index for w in plan.pass1] == list(range(len(plan.pass1)))
    done = []
    for i, w in enumerate(plan.pass1):
        assert len(w.slot_frame) == T and [w.slot_frame[s] for s in w.target_slots] == w.target_ids
        assert w.source_ids[:2] == ins  # every window starts from the ground-truth inputs
        if strategy == "gt":
            assert set(w.source_ids) == set(ins)
        else:
            assert set(w.source_ids) - set(ins) <= set(done)  # only frames generated earlier
            assert i == 0 or set(w.source_ids) - set(ins), i  # later windows do read earlier outputs
        done += w.target_ids
    # the default is the reference's: strategy "gt"
    assert [w.target_ids for w in pipeline.plan_views(c2ws, ins, T=T).pass1] == \
        [w.target_ids for w in pipeline.plan_views(c2ws, ins, T=T, chunk_strategy="gt").pass1]


def _run_views(group=None, strategy="gt", n=30, **kw):
    from test_pipeline_cpu import _fake_net
    from seva import pipeline
    c2ws, Ks, lat, tok = _scene(n)
    return pipeline.run_views(_fake_net, lat, c2ws, Ks, [0], clip_token=tok, T=8, num_steps=2, seed=23, device="cpu",
                              chunk_strategy=strategy, group=group, **kw)


@pytest.mark.parametrize("strategy", ["gt", "gt-nearest"])
def test_run_views_equals_a_hand_written_loop_of_run_window(strategy, monkeypatch):
    from test_pipeline_cpu import _fake_net, _patch_cpu
    from seva import pipeline
    _patch_cpu(monkeypatch)
    n, T, seed = 30, 8, 23
    c2ws, Ks, lat, tok = _scene(n)
    res = _run_views(strategy=strategy, n=n)
    plan = pipeline.plan_views(c2ws, [0], T=T, chunk_strategy=strategy)
    assert [w.target_ids for w in res["plan"].pass1] == [w.target_ids for w in plan.pass1] and res["plan"].pass2 == []
    g0 = torch.Generator().manual_seed(seed)
    noises = [torch.randn((T, 4, 8, 8), generator=g0) for _ in plan.pass1]
    latents_of = {0: lat[0]}
    for w in plan.pass1:
        z = pipeline.run_window(w, latents_of, _fake_net, c2ws, Ks, hw=(8, 8), num_steps=2, cfg=2.0, cfg_min=1.2, guider=1,
                                camera_scale=2.0, noise=noises[w.global_index],
                                step_seed=(seed * 1000003 + 7919 * (w.global_index + 1)) & 0x7FFFFFFFFFFF, clip_token=tok, device="cpu")
        for fid, slot in zip(w.target_ids, w.target_slots):
            latents_of[fid] = z[slot]
    want = torch.stack([latents_of[f] for f in range(n)])
    assert res["latents"].shape == (n, 4, 8, 8) and torch.equal(res["latents"], want)
    assert torch.equal(res["latents"][0], lat[0]) and all(float(res["latents"][f].abs().max()) > 0 for f in range(1, n))


def test_rgb_handoff_outputs_a_frames_own_sample(monkeypatch):
    """handoff='rgb' in one pass: later windows read encode(decode(sample)), the OUTPUT is the sample itself (the reference
    decodes it directly), so the result differs from the latent hand-off only through what later windows read."""
    from test_pipeline_cpu import _patch_cpu
    _patch_cpu(monkeypatch)

    class FakeAE:
        def decode(self, z):
            return torch.tanh(z[:, :3] * 0.5 + 0.1 * z[:, 3:4])

        def encode(self, x):
            return torch.cat([x * 1.5, x.mean(1, keepdim=True)], 1)

    a = _run_views(strategy="gt-nearest", ae=FakeAE(), handoff="rgb")
    b = _run_views(strategy="gt-nearest")
    first = a["plan"].pass1[0].target_ids
    assert torch.equal(a["latents"][first], b["latents"][first])  # the first window read inputs only: its own samples
    assert torch.equal(a["rgb"], FakeAE().decode(a["latents"]))
    seen = a["anchor_latents"][first[0]]  # what later windows conditioned on went through the round trip
    assert torch.allclose(seen[3], seen[:3].mean(0) / 1.5, atol=1e-6) and not torch.equal(seen, a["latents"][first[0]])
    later = a["plan"].pass1[-1].target_ids
    assert not torch.equal(a["latents"][later], b["latents"][later])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    from test_pipeline_cpu import _patch_cpu
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _patch_cpu()
    res = _run_views(strategy="gt")
    q.put((rank, res["latents"].numpy() if "latents" in res else None))
    dist.destroy_process_group()


def test_two_rank_sharded_views_equal_single_process(monkeypatch):
    from conftest import PKG
    from test_pipeline_cpu import _patch_cpu
    here = os.path.dirname(os.path.abspath(__file__))
    os.environ["PYTHONPATH"] = os.pathsep.join([PKG, here, os.environ.get("PYTHONPATH", "")])
    _patch_cpu(monkeypatch)
    ref = _run_views(strategy="gt")["latents"]
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert res[1][1] is None and torch.equal(torch.from_numpy(res[0][1]), ref)


# ---- run_scene: one-pass mode and targets ----------------------------------------------------------------------------------
def _scene_args():
    from conftest import load_golden
    from seva import synthetic as synth
    g = load_golden("g12_frames")
    n, ids = 12, [0, 1]
    images = [g["src_s1"].numpy(), g["src_s2"]]
    tok = torch.randn(1024, generator=torch.Generator().manual_seed(5))
    return g, n, ids, images, synth.orbit_c2w(n), synth.default_K(n), tok / tok.norm()


@pytest.mark.parametrize("prior", [False, True])
def test_run_scene_scores_targets_in_both_modes(prior, fake, monkeypatch):
    from test_frames_cpu import _ToyAE
    from test_pipeline_cpu import _fake_net, _patch_cpu
    from seva import frames, metrics, pipeline
    _patch_cpu(monkeypatch)
    g, n, ids, images, c2ws, Ks, tok = _scene_args()
    ae = _ToyAE()
    kw = dict(size=(48, 32), clip_token=tok, T=4, num_steps=2, device="cpu", use_traj_prior=prior)
    plain = pipeline.run_scene(_fake_net, ae, images, c2ws, Ks, ids, **kw)
    assert "metrics" not in plain and plain["frames"].shape == (n, 32, 48, 3)
    if not prior:
        assert plain["plan"].pass2 == [] and len(plain["plan"].pass1) >= 4
        lat = torch.stack([ae.encode(frames.load_img_and_K(im, (48, 32), device="cpu")[0])[0] for im in images])
        Kn = Ks.clone()
        for i, fid in enumerate(ids):
            K = frames.load_img_and_K(images[i], (48, 32), K=Ks[fid], device="cpu")[1]
            Kn[fid] = K / K.new_tensor([48, 32, 1.0])[:, None]
        byhand = pipeline.run_views(_fake_net, lat, c2ws, Kn, ids, clip_token=tok, T=4, num_steps=2, device="cpu")
        assert torch.equal(plain["latents"], byhand["latents"])
        assert torch.equal(plain["frames"], frames.to_uint8(ae.decode(byhand["latents"])))
    # held-out pictures: an RGBA array and an RGB tensor, loaded like the inputs
    targets = {7: g["src_s2"], 3: g["src_s1"].numpy()}
    res = pipeline.run_scene(_fake_net, ae, images, c2ws, Ks, ids, targets=targets, **kw)
    assert torch.equal(res["frames"], plain["frames"])
    m = res["metrics"]
    assert set(m) == {"frame_ids", "sse", "psnr", "ssim"} and m["frame_ids"] == [3, 7]
    want_u8 = torch.cat([frames.to_uint8(frames.load_img_and_K(targets[f], (48, 32), device="cpu")[0]) for f in (3, 7)])
    want = metrics.compare(res["frames"][[3, 7]], want_u8)
    for k in ("sse", "psnr", "ssim"):
        assert torch.equal(m[k], want[k]), k
    assert (m["sse"] > 0).all() and torch.isfinite(m["psnr"]).all() and (m["ssim"] < 1).all()
    # a run scored against its own frames: exactly inf / 1.0 ...
    me = metrics.compare(res["frames"], res["frames"].clone())
    assert int(me["sse"].abs().max()) == 0 and torch.isinf(me["psnr"]).all() and torch.equal(me["ssim"], torch.ones(n, dtype=torch.float64))
    # ... and through `targets=` what the loader makes of them: pictures go uint8 -> [-1, 1] -> uint8 like the inputs, and the
    # reference's two rules (v / 255 * 2 - 1, then (v + 1) / 2 * 255 truncated) give bytes 1..63 back one lower
    own_t = {f: res["frames"][f] for f in (2, 5, 11)}
    own = pipeline.run_scene(_fake_net, ae, images, c2ws, Ks, ids, targets=own_t, **kw)["metrics"]
    back = torch.cat([frames.to_uint8(frames.load_img_and_K(own_t[f], (48, 32), device="cpu")[0]) for f in (2, 5, 11)])
    dark = (res["frames"][[2, 5, 11]] >= 1) & (res["frames"][[2, 5, 11]] <= 63)
    assert torch.equal(back, res["frames"][[2, 5, 11]] - dark.to(torch.uint8))
    assert own["frame_ids"] == [2, 5, 11] and torch.equal(own["sse"], dark.sum(dim=(1, 2, 3)))
    assert torch.equal(own["ssim"], metrics.compare(res["frames"][[2, 5, 11]], back)["ssim"]) and (own["ssim"] > 0.99).all()


def test_two_pass_scene_is_unchanged_by_the_new_arguments(fake, monkeypatch):
    """`use_traj_prior=True` (the default) is today's two-pass run: the same plan, the same call of `run_trajectory`."""
    from test_frames_cpu import _ToyAE
    from test_pipeline_cpu import _fake_net, _patch_cpu
    from seva import frames, pipeline
    _patch_cpu(monkeypatch)
    g, n, ids, images, c2ws, Ks, tok = _scene_args()
    ae = _ToyAE()
    kw = dict(size=(48, 32), clip_token=tok, T=4, num_steps=2, device="cpu")
    a = pipeline.run_scene(_fake_net, ae, images, c2ws, Ks, ids, **kw)
    b = pipeline.run_scene(_fake_net, ae, images, c2ws, Ks, ids, use_traj_prior=True, **kw)
    assert torch.equal(a["frames"], b["frames"]) and torch.equal(a["latents"], b["latents"])
    assert len(a["plan"].pass2) >= 1
    lat = torch.stack([ae.encode(frames.load_img_and_K(im, (48, 32), device="cpu")[0])[0] for im in images])
    Kn = Ks.clone()
    for i, fid in enumerate(ids):
        K = frames.load_img_and_K(images[i], (48, 32), K=Ks[fid], device="cpu")[1]
        Kn[fid] = K / K.new_tensor([48, 32, 1.0])[:, None]
    traj = pipeline.run_trajectory(_fake_net, lat, c2ws, Kn, ids, clip_token=tok, T=4, num_steps=2, device="cpu", ae=ae)
    assert torch.equal(a["latents"], traj["latents"]) and torch.equal(a["rgb"], traj["rgb"])
    c = pipeline.run_scene(_fake_net, ae, images, c2ws, Ks, ids, use_traj_prior=False, **kw)
    assert not torch.equal(a["latents"], c["latents"])
