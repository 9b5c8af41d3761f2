"""`seva_frame_metrics` on the device (`seva.metrics`, `ops.frame_metrics`): exact squared error and SSIM against the fp64
expression on the cases of tests/metric_cases.py, both input kinds; invariance to n, to the image pitch and to repetition;
guards around every output; and the one-pass `run_scene(use_traj_prior=False, targets=...)` on the tiny synthetic model."""
import pytest
import torch

import metric_cases as MC

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from seva import _native
    _native.load()
    return torch.device("cuda:0")


@pytest.mark.parametrize("case", [c[0] for c in MC.all_cases()])
def test_sse_exact_and_ssim_within_the_bounds_of_use(case, dev):
    from seva import metrics
    a, b = next((a, b) for cid, a, b in MC.all_cases() if cid == case)
    sse, ssim, smap = MC.reference(case)
    got = {}
    for kind, (xa, xb) in {"u8": (a, b), "f32": (MC.to_f32(a), MC.to_f32(b))}.items():
        m = metrics.compare(xa.to(dev), xb.to(dev), ssim_map=True)
        got[kind] = m
        e_frame = float((m["ssim"].cpu() - ssim).abs().max())
        e_map = float((m["ssim_map"].cpu().double() - smap).abs().max())
        print(f"{case} {kind}: frame err {e_frame:.3e} map err {e_map:.3e}")
        assert m["sse"].dtype == torch.int64 and torch.equal(m["sse"].cpu(), sse), (case, kind)
        assert e_frame < MC.FRAME_TOL and e_map < MC.MAP_TOL, (case, kind, e_frame, e_map)
    for k in ("sse", "ssim", "ssim_map", "psnr"):
        assert torch.equal(got["u8"][k], got["f32"][k]), k  # both kinds score the same integers
    # SSE-only call: the same squared error, no SSIM work
    assert torch.equal(metrics.compare(a.to(dev), b.to(dev), ssim=False)["sse"].cpu(), sse)


def test_a_frame_against_itself_is_exactly_one(dev):
    from seva import metrics
    for name in ("noise", "smooth_pm6", "white_half_black"):
        for x in MC.pair(name):
            for t in (x.to(dev), MC.to_f32(x).to(dev)):
                m = metrics.compare(t, t.clone(), ssim_map=True)
                assert int(m["sse"].abs().max()) == 0 and torch.isinf(m["psnr"]).all()
                assert torch.equal(m["ssim"], torch.ones(MC.N, dtype=torch.float64, device=dev))
                assert torch.equal(m["ssim_map"], torch.ones_like(m["ssim_map"]))


def test_fp32_kind_equals_u8_kind_of_to_uint8_including_nan_and_out_of_range(dev):
    from seva import frames, metrics
    g = torch.Generator().manual_seed(11)
    a = torch.rand((MC.N, 3, MC.H0, MC.W0), generator=g) * 2.6 - 1.3   # beyond [-1, 1] on both sides
    b = (a + 0.2 * torch.randn(a.shape, generator=g)).contiguous()
    a[0, 1, 5, 7] = float("nan")
    b[1, 2, 36, 52] = float("nan")
    a[2, 0, 0, 0], b[2, 0, 0, 1] = float("inf"), float("-inf")
    a, b = a.to(dev), b.to(dev)
    ua, ub = frames.to_uint8(a), frames.to_uint8(b)
    assert int(ua.min()) == 0 and int(ua.max()) == 255
    mf = metrics.compare(a, b, ssim_map=True)
    mu = metrics.compare(ua, ub, ssim_map=True)
    for k in ("sse", "ssim", "ssim_map"):
        assert torch.equal(mf[k], mu[k]), k
    assert torch.equal(mu["sse"].cpu(), MC.sse_i64(ua.cpu(), ub.cpu()))


def test_independent_of_n_pitch_and_repetition(dev):
    from seva import metrics
    for name in ("noise", "smooth_pm6"):
        a, b = (t.to(dev) for t in MC.pair(name))
        fa, fb = MC.to_f32(a.cpu()).to(dev), MC.to_f32(b.cpu()).to(dev)
        full = metrics.compare(a, b, ssim_map=True)
        again = metrics.compare(a, b, ssim_map=True)
        for k in ("sse", "ssim", "ssim_map"):
            assert torch.equal(full[k], again[k]), k
        for i in range(MC.N):  # n = 1 slices
            for xa, xb in ((a, b), (fa, fb)):
                one = metrics.compare(xa[i:i + 1], xb[i:i + 1], ssim_map=True)
                for k in ("sse", "ssim", "ssim_map"):
                    assert torch.equal(one[k][0], full[k][i]), (k, i)
        # a padded image pitch (a misaligned one for the bytes: 3 * 37 * 53 + 5), one operand only and both
        for xa, xb, pad in ((a, b, 5), (fa, fb, 7)):
            flat = lambda t: t.reshape(MC.N, -1)
            pa = torch.full((MC.N, flat(xa).shape[1] + pad), 99, dtype=xa.dtype, device=dev)
            pb = torch.full_like(pa, 77)
            pa[:, :flat(xa).shape[1]] = flat(xa)
            pb[:, :flat(xb).shape[1]] = flat(xb)
            va, vb = pa[:, :flat(xa).shape[1]].view(xa.shape), pb[:, :flat(xb).shape[1]].view(xb.shape)
            assert va.stride(0) == flat(xa).shape[1] + pad
            for ya, yb in ((va, xb), (va, vb)):
                m = metrics.compare(ya, yb, ssim_map=True)
                for k in ("sse", "ssim", "ssim_map"):
                    assert torch.equal(m[k], full[k]), (k, pad)


def test_guards_around_every_output_and_the_workspace(dev):
    from seva import ops
    for (H, W) in ((MC.H0, MC.W0), (11, 11), (64, 96)):
        a, b = (t.to(dev) for t in MC.pair("noise", H, W))
        n = a.shape[0]
        ws_n = ops.frame_metrics_workspace_numel(n, H, W)
        assert ws_n > 0

        def guarded(numel, dtype, fill):
            buf = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device=dev)
            return buf, buf[GUARD:GUARD + numel]

        sse_b, sse = guarded(n, torch.int64, -7)
        sum_b, ssum = guarded(n, torch.float64, -3.0)
        map_b, smap = guarded(n * 3 * (H - 10) * (W - 10), torch.float32, -5.0)
        ws_b, ws = guarded(ws_n, torch.uint8, 0xA5)
        ops.frame_metrics(a, b, sse, ssum, smap.view(n, 3, H - 10, W - 10), ws)
        torch.cuda.synchronize()
        for buf, fill in ((sse_b, -7), (sum_b, -3.0), (map_b, -5.0), (ws_b, 0xA5)):
            assert bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())
        assert torch.equal(sse.cpu(), MC.sse_i64(a.cpu(), b.cpu()))
        assert bool((smap != -5.0).all()) and bool((ssum != -3.0).all())
        # SSE only: ssim outputs untouched, no size limit
        sse.fill_(-7)
        ops.frame_metrics(a[:, :7, :9].contiguous(), b[:, :7, :9].contiguous(), sse, None, None, ws)
        assert torch.equal(sse.cpu(), MC.sse_i64(a[:, :7, :9].cpu(), b[:, :7, :9].cpu()))
        assert bool((ws_b[:GUARD] == 0xA5).all()) and bool((ws_b[-GUARD:] == 0xA5).all())


def test_small_frames_with_ssim_are_refused_by_the_library(dev):
    from seva import _native, metrics
    a, b = (t.to(dev) for t in MC.pair("noise"))
    for sl in ((slice(None), slice(0, 10)), (slice(None), slice(None), slice(0, 10))):
        with pytest.raises(_native.SevaNativeError, match="11"):
            metrics.compare(a[sl].contiguous(), b[sl].contiguous())
    with pytest.raises(_native.SevaNativeError):
        metrics.compare(a.cpu(), b.cpu())
    assert torch.equal(metrics.compare(a, b, ssim=False)["sse"].cpu(), MC.sse_i64(a.cpu(), b.cpu()))  # the library still works


def test_one_pass_scene_with_targets_on_the_tiny_model(dev):
    """run_scene(use_traj_prior=False, targets=...) on the tiny synthetic UNet with a linear stand-in for the VAE (T = 4, 2 steps):
    the metrics are `compare` on the returned frames, the frames are run_views + decode + to_uint8 composed by hand."""
    from test_frames_cpu import _ToyAE
    from test_model_gpu import _build
    from seva import frames, metrics, pipeline
    from seva import synthetic as synth
    from seva.model import SGMWrapper
    net, _ = _build("tiny", dev)
    wrap = SGMWrapper(net)
    n, ids, size, T = 8, [0, 4], (128, 128), 4
    c2ws, Ks = synth.orbit_c2w(n), synth.default_K(n)
    g = torch.Generator().manual_seed(9)
    images = [torch.randint(0, 256, (150, 140, 3), generator=g, dtype=torch.int64).to(torch.uint8) for _ in ids]
    targets = {f: torch.randint(0, 256, (128, 160, 3), generator=g, dtype=torch.int64).to(torch.uint8) for f in (6, 1)}
    tok = torch.randn(1024, generator=g)
    tok = (tok / tok.norm()).to(dev)
    ae = _ToyAE()
    kw = dict(clip_token=tok, T=T, num_steps=2, device=dev)
    with torch.no_grad():
        res = pipeline.run_scene(wrap, ae, images, c2ws, Ks, ids, size=size, use_traj_prior=False, targets=targets, **kw)
        assert res["plan"].pass2 == [] and len(res["plan"].pass1) == 3
        assert res["frames"].shape == (n, 128, 128, 3) and res["frames"].dtype == torch.uint8
        m = res["metrics"]
        assert m["frame_ids"] == [1, 6]
        want_u8 = torch.cat([frames.to_uint8(frames.load_img_and_K(targets[f], size, device=dev)[0]) for f in (1, 6)])
        want = metrics.compare(res["frames"][[1, 6]], want_u8)
        for k in ("sse", "psnr", "ssim"):
            assert torch.equal(m[k], want[k]), k
        assert torch.equal(m["sse"].cpu(), MC.sse_i64(res["frames"][[1, 6]].cpu(), want_u8.cpu()))
        assert torch.isfinite(m["psnr"]).all() and (m["ssim"].abs() < 1).all()
        # composed by hand
        x = torch.cat([frames.load_img_and_K(im, size, K=Ks[f], device=dev)[0] for im, f in zip(images, ids)])
        Kn = Ks.clone()
        for im, f in zip(images, ids):
            K = frames.load_img_and_K(im, size, K=Ks[f], device=dev)[1]
            Kn[f] = K / K.new_tensor([128, 128, 1.0])[:, None]
        byhand = pipeline.run_views(wrap, ae.encode(x), c2ws, Kn, ids, **kw)
    assert torch.equal(res["latents"], byhand["latents"]) and torch.isfinite(res["latents"]).all()
    assert torch.equal(res["frames"], frames.to_uint8(ae.decode(byhand["latents"])))
    assert all(float(res["latents"][f].abs().max()) > 0 for f in range(n))
