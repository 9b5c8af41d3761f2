"""LPIPS (`seva.metrics.LPIPS`, `seva._lpips_engine`) without a GPU: the weight loader, the unchanged defaults of `compare` and
`run_scene`, the binding, and the engine on the torch emulations of its operators (tests/fake_ops.py's convolution beside
tests/fake_lpips_ops.py) against the fp64 restatement of the published definition (tests/lpips_ref.py).

That last run yields the F16-OPERAND FLOOR: what rounding the activations and weights to f16 (fp32 accumulation, fp32 distance
arithmetic as the contract states it) costs against fp64 on unrounded weights, per case: the worst absolute error over the
frames of the five layer means and of their sum.  Measured (printed by the test; the last digits depend on the order in which
the host's fp32 convolution accumulates):

    40 x 56   4.862e-08   (scores 2.9e-3 and 3.1e-3 on the synthetic weights: 1.6e-5 of the score)
    32 x 32   1.818e-07   (5.9e-5 of the score)
    64 x 48   5.819e-08   (1.8e-5 of the score)

tests/test_lpips_gpu.py holds the HIP path to twice these figures (`lpips_ref.F16_FLOOR`)."""
import os
import re

import pytest
import torch

import lpips_ref as R
from conftest import ROOT


@pytest.fixture
def cpu_engine(monkeypatch):
    import fake_frame_ops
    import fake_lpips_ops
    import fake_metric_ops
    import seva.ops as ops
    from seva import _lpips_engine
    monkeypatch.setattr(_lpips_engine, "ops", fake_lpips_ops.OPS)
    monkeypatch.setattr(_lpips_engine, "require_cuda", lambda *a: None)
    monkeypatch.setattr(_lpips_engine.LpipsEngine, "_resolve_device", staticmethod(lambda w: torch.device("cpu")))
    monkeypatch.setattr(ops, "frame_metrics", fake_metric_ops.frame_metrics)
    monkeypatch.setattr(ops, "image_area_crop", fake_frame_ops.image_area_crop)
    monkeypatch.setattr(ops, "rgb_to_u8", fake_frame_ops.rgb_to_u8)


# ---- weights ----------------------------------------------------------------------------------------------------------------
def test_key_set_is_the_public_one_and_loading_is_strict():
    from seva import metrics
    w = metrics.LpipsWeights()
    keys = set(w.state_dict())
    want = {f"features.{i}.{p}" for i in R.CONVS for p in ("weight", "bias")} | {f"lin{k}.model.1.weight" for k in range(5)}
    assert keys == want
    cin = 3
    for i, c in zip(R.CONVS, (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)):
        assert w.state_dict()[f"features.{i}.weight"].shape == (c, cin, 3, 3) and w.state_dict()[f"features.{i}.bias"].shape == (c,)
        cin = c
    for k, c in enumerate(R.WIDTHS):
        assert w.state_dict()[f"lin{k}.model.1.weight"].shape == (1, c, 1, 1)
    sd = dict(R.state_dict())
    w.load_state_dict(sd)
    assert all(torch.equal(w.state_dict()[k], sd[k]) for k in sd)
    assert all(float(sd[f"lin{k}.model.1.weight"].min()) >= 0 for k in range(5))
    for bad in ({k: v for k, v in sd.items() if k != "features.14.bias"},               # missing
                {**sd, "features.30.weight": torch.zeros(1)},                             # unexpected
                {**sd, "lin2.model.1.weight": torch.zeros(1, 128, 1, 1)},                  # misshapen
                {**sd, "features.5.weight": sd["features.5.weight"][:, :, :1, :1]}):
        with pytest.raises(RuntimeError):
            metrics.LpipsWeights().load_state_dict(bad)


def test_loader_reads_local_files_in_both_layouts(tmp_path, monkeypatch):
    from seva import metrics
    monkeypatch.delenv("SEVA_LPIPS_VGG_PATH", raising=False)
    monkeypatch.delenv("SEVA_LPIPS_LIN_PATH", raising=False)
    sd = R.state_dict()
    same = lambda w: all(torch.equal(w.state_dict()[k], sd[k]) for k in sd)
    with pytest.raises(ValueError, match="SEVA_LPIPS_VGG_PATH"):
        metrics.load_lpips_weights()
    # one merged file, the package's `net.slice{j}.{i}.` prefix and its scaling-layer buffers
    slice_of = {0: 1, 2: 1, 5: 2, 7: 2, 10: 3, 12: 3, 14: 3, 17: 4, 19: 4, 21: 4, 24: 5, 26: 5, 28: 5}
    merged = {(f"net.slice{slice_of[int(k.split('.')[1])]}.{k.split('.', 1)[1]}" if k.startswith("features.") else k): v
              for k, v in sd.items()}
    merged["scaling_layer.shift"], merged["scaling_layer.scale"] = torch.zeros(1, 3, 1, 1), torch.ones(1, 3, 1, 1)
    assert "net.slice3.14.bias" in merged and not any(k.startswith("features.") for k in merged)
    one = str(tmp_path / "merged.pth")
    torch.save(merged, one)
    assert same(metrics.load_lpips_weights(one))
    # a torchvision VGG-16 file (with its classifier) beside the linear-layer file
    vgg = {k: v for k, v in sd.items() if k.startswith("features.")}
    vgg["classifier.0.weight"], vgg["classifier.0.bias"] = torch.zeros(4, 4), torch.zeros(4)
    lin = {k: v for k, v in sd.items() if k.startswith("lin")}
    pv, pl = str(tmp_path / "vgg16.pth"), str(tmp_path / "lin.pth")
    torch.save(vgg, pv)
    torch.save(lin, pl)
    assert same(metrics.load_lpips_weights(pv, pl))
    with pytest.raises(RuntimeError):  # the VGG file alone: the linear layers are missing
        metrics.load_lpips_weights(pv)
    with pytest.raises(ValueError, match="both files"):
        metrics.load_lpips_weights(one, pl)
    # paths from the environment
    monkeypatch.setenv("SEVA_LPIPS_VGG_PATH", pv)
    with pytest.raises(RuntimeError):
        metrics.load_lpips_weights()
    monkeypatch.setenv("SEVA_LPIPS_LIN_PATH", pl)
    assert same(metrics.load_lpips_weights())
    bad = dict(lin)
    bad.pop("lin4.model.1.weight")
    torch.save(bad, pl)
    with pytest.raises(RuntimeError, match="lin4"):
        metrics.load_lpips_weights()


def test_synthetic_weights_keep_activations_of_order_one():
    import torch.nn.functional as F
    sd = R.state_dict()
    a, _ = R.pair(40, 56)
    x = a.permute(0, 3, 1, 2).float() / 127.5 - 1.0
    for i in R.CONVS:
        x = F.relu(F.conv2d(x, sd[f"features.{i}.weight"], sd[f"features.{i}.bias"], padding=1))
        rms = float(x.pow(2).mean().sqrt())
        assert 0.05 < rms < 20.0, (i, rms)
        if i + 1 in R.POOL_AFTER:
            x = F.max_pool2d(x, 2, 2)


# ---- defaults unchanged, binding -------------------------------------------------------------------------------------------------
def test_compare_and_run_scene_without_lpips_are_unchanged(cpu_engine):
    import inspect

    import metric_cases as MC
    from seva import metrics, pipeline
    a, b = MC.pair("smooth_pm6")
    assert set(metrics.compare(a, b)) == {"sse", "mse", "psnr", "ssim"}
    assert set(metrics.compare(a, b, ssim=False)) == {"sse", "mse", "psnr"}
    assert set(metrics.compare(a, b, ssim_map=True)) == {"sse", "mse", "psnr", "ssim", "ssim_map"}
    assert inspect.signature(metrics.compare).parameters["lpips"].default is None
    assert inspect.signature(pipeline.run_scene).parameters["lpips"].default is None
    m = metrics.LPIPS(R.weights())
    x, y = R.pair(32, 32)
    with_l = metrics.compare(x, y, lpips=m)
    without = metrics.compare(x, y)
    assert set(with_l) == set(without) | {"lpips", "lpips_layers"}
    assert all(torch.equal(with_l[k], without[k]) for k in without)
    assert with_l["lpips"].dtype == torch.float64 and with_l["lpips"].shape == (R.N,) and with_l["lpips_layers"].shape == (R.N, 5)
    assert torch.equal(with_l["lpips"], with_l["lpips_layers"].sum(1)) and torch.equal(with_l["lpips"], m(x, y))


def test_run_scene_adds_lpips_only_when_asked(cpu_engine, monkeypatch):
    from test_frames_cpu import _ToyAE
    from test_pipeline_cpu import _fake_net, _patch_cpu, _scene
    from seva import frames, metrics, pipeline
    _patch_cpu(monkeypatch)
    n, ids, size = 8, [0, 4], (32, 32)
    c2ws, Ks, _, tok = _scene(n, 4)
    g = torch.Generator().manual_seed(9)
    images = [torch.randint(0, 256, (40, 36, 3), generator=g, dtype=torch.int64).to(torch.uint8) for _ in ids]
    targets = {f: torch.randint(0, 256, (32, 40, 3), generator=g, dtype=torch.int64).to(torch.uint8) for f in (6, 1)}
    kw = dict(clip_token=tok, T=4, num_steps=2, seed=23, device="cpu", size=size, use_traj_prior=False, targets=targets)
    m = metrics.LPIPS(R.weights())
    plain = pipeline.run_scene(_fake_net, _ToyAE(), images, c2ws, Ks, ids, **kw)
    scored = pipeline.run_scene(_fake_net, _ToyAE(), images, c2ws, Ks, ids, lpips=m, **kw)
    assert set(plain["metrics"]) == {"frame_ids", "sse", "psnr", "ssim"}
    assert set(scored["metrics"]) == set(plain["metrics"]) | {"lpips"}
    assert torch.equal(plain["frames"], scored["frames"])
    assert all(torch.equal(plain["metrics"][k], scored["metrics"][k]) for k in ("sse", "psnr", "ssim"))
    want = torch.cat([frames.to_uint8(frames.load_img_and_K(targets[f], size, device="cpu")[0]) for f in (1, 6)])
    assert torch.equal(scored["metrics"]["lpips"], m(scored["frames"][[1, 6]], want))
    assert (scored["metrics"]["lpips"] > 0).all()


def test_new_symbols_in_header_binding_and_makefile():  # (header against binding: tests/test_abi_cpu.py)
    mk = open(os.path.join(ROOT, "stable-virtual-camera_amd", "csrc", "Makefile")).read()
    assert "lpips.hip" in re.search(r"^SRCS\s*:=\s*(.+)$", mk, re.M).group(1).split()
    assert re.search(r"^FLAGS_lpips\s*:=.*-ffp-contract=off", mk, re.M)


def test_no_cpu_fallback_and_argument_checks(cpu_engine, monkeypatch):
    from seva import _native, metrics
    m = metrics.LPIPS(R.weights())
    a, b = R.pair(32, 32)
    for bad in ((a, b[:2]), (a, R.to_f32(b)), (a.float(), b.float()), (a[0], b[0])):
        with pytest.raises(ValueError):
            m(*bad)
    for sl in ((slice(None), slice(0, 31)), (slice(None), slice(None), slice(0, 31))):
        with pytest.raises(ValueError, match="32"):
            m(a[sl].contiguous(), b[sl].contiguous())
    with pytest.raises(ValueError):
        metrics.LPIPS(R.weights(), chunk_size=0).engine()
    monkeypatch.undo()  # the real engine: weights on the CPU are refused, nothing is computed in torch
    with pytest.raises(_native.SevaNativeError):
        metrics.LPIPS(R.weights())(a, b)


# ---- the engine on the emulated operators ------------------------------------------------------------------------------------------
def test_fake_operators_follow_the_contract():
    """The emulation itself, on what can be said without a GPU: the padded operand, torch's ReLU / max-pool (odd sizes, NaN),
    the distance against fp64, exact zero and symmetry."""
    import torch.nn.functional as F

    import fake_lpips_ops as FL
    g = torch.Generator().manual_seed(3)
    u8 = torch.randint(0, 256, (2, 5, 7, 3), generator=g, dtype=torch.int64).to(torch.uint8)
    out = torch.full((2, 5, 7, 64), 9.0, dtype=torch.float16)
    FL.lpips_prepare(u8, out)
    assert int((out[..., 3:] != 0).sum()) == 0
    want = ((u8.double() / 127.5 - 1.0) - torch.tensor(R.SHIFT, dtype=torch.float64)) / torch.tensor(R.SCALE, dtype=torch.float64)
    assert float((out[..., :3].double() - want).abs().max()) < 2.0 ** -10 * 2.3  # one f16 rounding of |x| < 2.3 (+ fp32 noise)
    out2 = torch.empty_like(out)
    FL.lpips_prepare(R.to_f32(u8), out2)
    assert torch.equal(out, out2)
    for (h, w) in ((5, 7), (6, 4), (2, 3)):
        x = torch.randn((2, h, w, 64), generator=g).half()
        x[0, 1, 1, 5] = float("nan")
        r, p = torch.empty_like(x), torch.empty((2, h // 2, w // 2, 64), dtype=torch.float16)
        FL.lpips_relu_pool(x, r, p)
        tr = F.relu(x.float())
        tp = F.max_pool2d(tr.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
        assert torch.equal(r.float().nan_to_num(7.0), tr.nan_to_num(7.0)) and torch.equal(p.float().nan_to_num(7.0), tp.nan_to_num(7.0))
        assert bool(torch.isnan(r[0, 1, 1, 5])) and bool(torch.isnan(p[0, 0, 0, 5])) and int(torch.isnan(p).sum()) == 1
    for C in (64, 512):
        fa, fb = torch.randn((2, 300, C), generator=g).relu().half(), torch.randn((2, 300, C), generator=g).relu().half()
        w = torch.rand(C, generator=g) / C
        o1, o2, o0 = (torch.empty(2, dtype=torch.float64) for _ in range(3))
        FL.lpips_layer(fa, fb, w, o1)
        FL.lpips_layer(fb, fa, w, o2)
        FL.lpips_layer(fa, fa.clone(), w, o0)
        ref = R.layer_sums_f64(fa, fb, w)
        assert torch.equal(o1, o2) and torch.equal(o0, torch.zeros(2, dtype=torch.float64))
        assert float(((o1 - ref) / ref).abs().max()) < 1e-6


@pytest.mark.parametrize("hw", R.CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_engine_on_emulated_operators_against_fp64(hw, cpu_engine):
    from seva import metrics
    H, W = hw
    a, b = R.pair(H, W)
    ref = R.reference(H, W)
    m = metrics.LPIPS(R.weights())
    got = m.layers(a, b)
    assert got.dtype == torch.float64 and got.shape == (R.N, 5)
    floor = max(float((got - ref).abs().max()), float((got.sum(1) - ref.sum(1)).abs().max()))
    print(f"{H}x{W}: lpips {ref.sum(1).tolist()} layers {ref[0].tolist()} f16-operand floor {floor:.3e}")
    # the last pair is identical: exactly 0 in every layer; the others are real distances
    assert torch.equal(got[R.N - 1], torch.zeros(5, dtype=torch.float64)) and float(ref[R.N - 1].abs().max()) == 0.0
    assert float(ref[:R.N - 1].sum(1).min()) > 1e-3
    # f16 operands carry 11 significant bits: one operand rounding is at most 2^-11 = 4.9e-4 of a value.  The floor must stay well
    # inside ONE such rounding of the score (3e-3 * 4.9e-4 = 1.5e-6) -- roundings of many features average out -- and it is what
    # lpips_ref.F16_FLOOR records for the GPU test
    assert floor < 1e-6, floor
    # symmetric, bit for bit
    assert torch.equal(m.layers(b, a), got)
    # both kinds of frames score the same integers
    assert torch.equal(m.layers(R.to_f32(a), R.to_f32(b)), got)
    # a pair's score does not depend on its chunk
    for cs in (1, 3):
        mc = metrics.LPIPS(R.weights(), chunk_size=cs)
        assert torch.equal(mc.layers(a, b), got), cs
        assert mc.engine()._chunk(R.N, H, W) == cs
    assert torch.equal(m(a, b), got.sum(1))


def test_default_chunk_keeps_the_arena_bounded():
    from seva import _lpips_engine as E
    per = E.pair_bytes(576, 576)
    assert 576 * 576 * 64 * 2 * 2 * 3 < per < 2 * 576 * 576 * 64 * 2 * 2 * 3   # three full-resolution 64-channel tensors dominate
    cs = max(1, E.ARENA_BYTES // per)
    assert 1 <= cs < 168 and cs * per <= E.ARENA_BYTES
    assert E.pair_bytes(32, 32) * 168 < E.ARENA_BYTES  # small frames: one pass
