"""LPIPS on the device (`seva.metrics.LPIPS`, csrc/lpips.hip): the preparation and ReLU / max-pool kernels bit for bit against the
torch expression, the layer-distance kernel against fp64 on the same f16 features, the whole score against the fp64 restatement of
the published definition (tests/lpips_ref.py) at the CPU test's cases, and `run_scene(..., targets, lpips=)` on the tiny synthetic
model.  Sentinel guards surround every output.

Bounds (none comes from the code under test):
  layer kernel   4 x the error of the contract's torch emulation (tests/fake_lpips_ops.py) against fp64 on the same features,
                 per case, computed here on the host: relative 1.2e-8 .. 7.9e-8 over C in 64 .. 512, hw in 4, 35, 1120 (fp32
                 arithmetic per pixel, fp64 sums).  The margin covers reduction order only.
  end to end     2 x the f16-operand floor of tests/test_lpips_cpu.py:
                 F16_FLOOR = {(40, 56): 4.862e-08, (32, 32): 1.818e-07, (64, 48): 5.819e-08}   (lpips_ref.F16_FLOOR)
                 the worst absolute error, over the frames, of the five layer means and of their sum, of the engine on emulated
                 operators (f16 operands, fp32 accumulation) against fp64; scores are 2.9e-3 .. 3.3e-3.  The margin covers the
                 MFMA accumulation order."""
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
SIZES = ((5, 7), (6, 4), (2, 3))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from seva import _native
    _native.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    from seva import metrics
    return metrics.LPIPS(R.weights()).to(dev)


def _guarded(numel, dtype, fill, dev):
    """(whole buffer, the numel elements between two guards of GUARD elements); numel * itemsize and GUARD keep 16-byte alignment"""
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + numel]


def _intact(buf, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


def _same(x, y):
    """equal, a NaN equal to a NaN"""
    return torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(x.nan_to_num(7.0), y.nan_to_num(7.0))


# ---- preparation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", SIZES + ((33, 20),), ids=lambda s: f"{s[0]}x{s[1]}")
def test_prepare_equals_the_torch_expression(hw, dev):
    import fake_lpips_ops as FL
    from seva import frames, ops
    H, W = hw
    n = 3
    g = torch.Generator().manual_seed(50 + H)
    u8 = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.int64).to(torch.uint8)
    u8[0, 0, 0], u8[0, -1, -1] = torch.tensor([0, 255, 128], dtype=torch.uint8), torch.tensor([255, 0, 127], dtype=torch.uint8)
    want = torch.zeros((n, H, W, 64), dtype=torch.float16)
    want[..., :3] = FL.prepared(u8)  # ((u8 / 127.5f - 1.0f) - shift) / scale, every operation rounded, one RNE to f16
    f32 = torch.rand((n, 3, H, W), generator=g) * 2.6 - 1.3   # beyond [-1, 1] on both sides
    f32[1, 2, 1, 1] = float("nan")
    f32 = f32.to(dev)
    want_f = torch.zeros_like(want)
    want_f[..., :3] = FL.prepared(frames.to_uint8(f32).cpu())
    for src, exp, pad in ((u8.to(dev), want, 0), (u8.to(dev), want, 5), (f32, want_f, 0), (f32, want_f, 7)):
        if pad:  # a padded image pitch (a misaligned one for the bytes)
            flat = src.reshape(n, -1)
            wide = torch.full((n, flat.shape[1] + pad), 99, dtype=src.dtype, device=dev)
            wide[:, :flat.shape[1]] = flat
            src = wide[:, :flat.shape[1]].view(src.shape)
            assert src.stride(0) == flat.shape[1] + pad
        buf, out = _guarded(n * H * W * 64, torch.float16, -3.0, dev)
        ops.lpips_prepare(src, out.view(n, H, W, 64))
        torch.cuda.synchronize()
        assert _intact(buf, -3.0)
        got = out.view(n, H, W, 64).cpu()
        assert int((got[..., 3:] != 0).sum()) == 0 and not bool(torch.signbit(got[..., 3:]).any())  # exactly +0
        assert torch.equal(got, exp), (hw, src.dtype, pad)


# ---- ReLU / max-pool -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [64, 128, 512])
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_relu_pool_equals_torch(hw, c, dev):
    from seva import ops
    h, w = hw
    n = 3
    g = torch.Generator().manual_seed(60 + h + c)
    x = torch.randn((n, h, w, c), generator=g).half()
    x[0, 1, 1, 5] = float("nan")          # torch: relu(NaN) = NaN, a NaN in a window is the window's maximum
    x[1, 0, 0, c - 1] = float("-inf")
    x[2, 0, 1, 0] = float("inf")
    x[1, 1, 2 if w > 2 else 1, 3] = -0.0
    xd = x.to(dev)
    want_r = F.relu(xd)
    want_p = F.max_pool2d(want_r.permute(0, 3, 1, 2).float(), 2, 2).permute(0, 2, 3, 1).half().contiguous()  # floor
    assert want_p.shape == (n, h // 2, w // 2, c) and bool(torch.isnan(want_p[0, 0, 0, 5]))
    for pool in (True, False):
        for inplace in (False, True):
            xbuf, xin = _guarded(x.numel(), torch.float16, -3.0, dev)
            xin.copy_(xd.view(-1))
            rbuf, r = (xbuf, xin) if inplace else _guarded(x.numel(), torch.float16, -5.0, dev)
            pbuf, p = _guarded(want_p.numel(), torch.float16, -9.0, dev)
            ops.lpips_relu_pool(xin.view(n, h, w, c), r.view(n, h, w, c), p.view(want_p.shape) if pool else None)
            torch.cuda.synchronize()
            assert _intact(xbuf, -3.0) and _intact(rbuf, -3.0 if inplace else -5.0) and _intact(pbuf, -9.0)
            assert _same(r.view(n, h, w, c), want_r), (hw, c, pool, inplace)
            if not inplace:
                assert _same(xin.view(n, h, w, c), xd)  # the input is only read
            if pool:
                assert _same(p.view(want_p.shape), want_p), (hw, c, inplace)
            else:
                assert bool((p == -9.0).all())


# ---- layer distance ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", R.LAYER_HWS)
@pytest.mark.parametrize("C", R.LAYER_CS)
def test_layer_distance_against_fp64_and_its_invariants(C, hw, dev):
    import fake_lpips_ops as FL
    from seva import ops
    fa, fb, w = R.layer_case(C, hw)
    n = fa.shape[0]
    ref = R.layer_sums_f64(fa, fb, w)
    emu = torch.empty(n, dtype=torch.float64)
    FL.lpips_layer(fa, fb, w, emu)
    tol = 4.0 * float((emu - ref).abs().max())
    a, b, wd = fa.to(dev), fb.to(dev), w.to(dev)
    ws_n = ops.lpips_layer_workspace_numel(n, hw)
    assert ws_n == n * ((hw + 255) // 256) * 8

    def run(x, y):
        m = x.shape[0]
        obuf, out = _guarded(m, torch.float64, -3.0, dev)
        wbuf, ws = _guarded(ops.lpips_layer_workspace_numel(m, hw), torch.uint8, 0xA5, dev)
        ops.lpips_layer(x, y, wd, out, ws)
        torch.cuda.synchronize()
        assert _intact(obuf, -3.0) and _intact(wbuf, 0xA5)
        return out.clone()

    got = run(a, b)
    err = float((got.cpu() - ref).abs().max())
    print(f"C={C} hw={hw}: sums {ref.tolist()} device err {err:.3e} emulation err {tol / 4:.3e} bit-equal to the emulation "
          f"{torch.equal(got.cpu(), emu)}")
    assert err <= tol, (C, hw, err, tol)
    assert torch.equal(run(a, b), got)                                              # repeated calls
    assert torch.equal(run(b, a), got)                                              # d(a, b) == d(b, a), bit for bit
    assert torch.equal(run(a, a.clone()), torch.zeros(n, dtype=torch.float64, device=dev))  # a frame against itself
    for i in range(n):                                                               # n = 1 slices equal the batch
        assert torch.equal(run(a[i:i + 1], b[i:i + 1])[0], got[i]), i
    # padded pair pitches (one operand only, and both), and the two halves of one tensor as the engine passes them
    wide = torch.full((n, hw * C + 24), 9.0, dtype=torch.float16, device=dev)
    wide[:, :hw * C] = a.view(n, -1)
    pa = wide[:, :hw * C].view(n, hw, C)
    assert pa.stride(0) == hw * C + 24
    assert torch.equal(run(pa, b), got) and torch.equal(run(b, pa), got)
    both = torch.cat([a, b])
    assert torch.equal(run(both[:n], both[n:]), got)
    out = torch.empty(n, dtype=torch.float64, device=dev)
    ops.lpips_layer(a, b, wd, out)   # workspace allocated by the wrapper
    assert torch.equal(out, got)


def test_layer_arguments_are_checked_by_the_library(dev):
    from seva import _native, ops
    fa, fb, w = (t.to(dev) for t in R.layer_case(64, 35))
    out = torch.empty(3, dtype=torch.float64, device=dev)
    with pytest.raises(_native.SevaNativeError, match="workspace"):
        d = _native.LpipsLayerDesc()
        d.fa, d.fb, d.w, d.out, d.workspace = fa.data_ptr(), fb.data_ptr(), w.data_ptr(), out.data_ptr(), fa.data_ptr()
        d.a_pitch_n = d.b_pitch_n = 35 * 64
        d.workspace_bytes, d.hw, d.n, d.C = 8, 35, 3, 64
        import ctypes
        _native.check(_native.load().seva_lpips_layer(ctypes.byref(d), _native.stream_ptr(dev)), "seva_lpips_layer")
    x96 = torch.zeros((3, 35, 96), dtype=torch.float16, device=dev)
    with pytest.raises(_native.SevaNativeError, match="C=96"):
        ops.lpips_layer(x96, x96, torch.zeros(96, device=dev), out)
    with pytest.raises(_native.SevaNativeError):
        ops.lpips_relu_pool(x96.view(3, 5, 7, 96), x96.view(3, 5, 7, 96))
    with pytest.raises(_native.SevaNativeError):
        ops.lpips_layer(fa.cpu(), fb.cpu(), w.cpu(), out.cpu())


# ---- the whole score ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", R.CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_lpips_against_the_fp64_restatement(hw, model, dev):
    from seva import metrics
    H, W = hw
    a, b = (t.to(dev) for t in R.pair(H, W))
    ref = R.reference(H, W)
    got = model.layers(a, b)
    assert got.dtype == torch.float64 and got.shape == (R.N, 5) and got.device.type == "cuda"
    err = max(float((got.cpu() - ref).abs().max()), float((got.cpu().sum(1) - ref.sum(1)).abs().max()))
    bound = 2.0 * R.F16_FLOOR[hw]
    print(f"{H}x{W}: lpips {got.sum(1).tolist()} reference {ref.sum(1).tolist()} err {err:.3e} bound {bound:.3e}")
    assert err <= bound, (hw, err, bound)
    assert torch.equal(got[R.N - 1], torch.zeros(5, dtype=torch.float64, device=dev))   # the identical pair
    assert torch.equal(model.layers(b, a), got)                                          # symmetric, bit for bit
    assert torch.equal(model.layers(a, b), got)                                          # repeatable
    # uint8 and fp32 frames of the same picture give bit-equal scores
    fa, fb = R.to_f32(a.cpu()).to(dev), R.to_f32(b.cpu()).to(dev)
    assert torch.equal(model.layers(fa, fb), got)
    m = metrics.compare(a, b, lpips=model)
    mf = metrics.compare(fa, fb, lpips=model)
    plain = metrics.compare(a, b)
    assert set(m) == set(plain) | {"lpips", "lpips_layers"} and all(torch.equal(m[k], plain[k]) for k in plain)
    assert torch.equal(m["lpips_layers"], got) and torch.equal(m["lpips"], got.sum(1)) and torch.equal(model(a, b), m["lpips"])
    assert torch.equal(mf["lpips"], m["lpips"])
    assert float((m["lpips"].cpu() - ref.sum(1)).abs().max()) <= bound
    # a pair's score does not depend on its chunk
    one = metrics.LPIPS(R.weights(), chunk_size=1).to(dev)
    assert torch.equal(one.layers(a, b), got)


def test_small_frames_and_cpu_tensors_are_refused(model, dev):
    from seva import _native, metrics
    a, b = (t.to(dev) for t in R.pair(32, 32))
    with pytest.raises(ValueError, match="32"):
        model(a[:, :31].contiguous(), b[:, :31].contiguous())
    with pytest.raises(_native.SevaNativeError):
        model(a.cpu(), b.cpu())
    with pytest.raises(_native.SevaNativeError):
        metrics.LPIPS(R.weights())(a, b)   # weights not on the device


def test_run_scene_with_targets_and_lpips_on_the_tiny_model(model, dev):
    """run_scene(use_traj_prior=False, targets=..., lpips=m) on the tiny synthetic UNet with a linear stand-in for the VAE (T = 4,
    2 steps): metrics["lpips"] is m(frames, targets), and everything else is what the run without `lpips` returns."""
    from test_frames_cpu import _ToyAE
    from test_model_gpu import _build
    from seva import frames, pipeline
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
    kw = dict(clip_token=tok, T=T, num_steps=2, device=dev, size=size, use_traj_prior=False, targets=targets)
    with torch.no_grad():
        res = pipeline.run_scene(wrap, _ToyAE(), images, c2ws, Ks, ids, lpips=model, **kw)
        plain = pipeline.run_scene(wrap, _ToyAE(), images, c2ws, Ks, ids, **kw)
    assert set(plain["metrics"]) == {"frame_ids", "sse", "psnr", "ssim"}
    assert set(res["metrics"]) == set(plain["metrics"]) | {"lpips"} and res["metrics"]["frame_ids"] == [1, 6]
    assert torch.equal(res["frames"], plain["frames"])
    assert all(torch.equal(res["metrics"][k], plain["metrics"][k]) for k in ("sse", "psnr", "ssim"))
    want_u8 = torch.cat([frames.to_uint8(frames.load_img_and_K(targets[f], size, device=dev)[0]) for f in (1, 6)])
    lp = res["metrics"]["lpips"]
    assert lp.dtype == torch.float64 and lp.shape == (2,) and torch.equal(lp, model(res["frames"][[1, 6]], want_u8))
    assert torch.isfinite(lp).all() and (lp > 0).all()
