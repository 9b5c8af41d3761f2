"""Windows of 33 to 96 views on the device: the temporal attention past one wave, the network, the trajectory driver.

A semi-dense scene's first pass is one window of all inputs + all anchors (T = 27 ... 96) and `interp-gt` widens the second pass
(T = 33, 53); the one-pass evaluation of 32 inputs runs T = 80 / 90.  Every other test stops at T = 25.  What changes with T:

  temporal attention   lq = lk = T, batch = (scene, pixel), tokens read through strides.  T <= 32: attn_kernel<1, 32>.  33 .. 64:
                       attn_kernel<4, 64> (two of its four waves own no row) or, knob attn_short2 = 1, attn_kernel<2, 64> on ONE
                       K/V buffer -- the same arithmetic per wave, so the same bits.  65 ..: attn_kernel<4, 64>, two key tiles.
  joint attention      lq = lk = T * hw: more tiles, the K/V split from 6144 keys on.
  everything else      rows = 2 T * hw: grids, arena, split-K workspaces.

a. `ops.attention` in the temporal layout against fp64 softmax (the bound of test_ops_gpu.py::test_attention_temporal_strided), plain
   and pre-scaled q, NaN-filled output between guard rows; the dense layout at 33 and 64 tokens.
b. Both routes of 32 < lq <= 64 give equal bits.
c. The tiny network layer by layer against the oracle at T = 33, 41, 64, 65, 90.
d. The 1.3B network against the reference at T = 41, 64, 65, 90 (tests/golden/g15_*, oracle/make_goldens_semidense.py); the README's
   bitwise promises at T = 41.
e. A semi-dense trajectory (12 inputs, 60 frames: windows of 21 and of 33) and a one-pass window of 90 through the driver.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import load_golden, rel_l2
from test_model_gpu import LAYER_TOL, NET_TOL, _build, _layer_table

QK_C = 0.125 * math.log2(math.e)
GUARD = 3  # rows of (S, C) before and after the output


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from seva import _native
    _native.load()
    return torch.device("cuda:0")


@pytest.fixture
def short2():
    """knob attn_short2 for one test; unset afterwards"""
    from seva import ops
    yield lambda v: ops.set_knob("attn_short2", int(v))
    ops.set_knob("attn_short2", -1)


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


# ------------------------------------------------------------------------------------------------------------ a. the kernel
TEMPORAL = [(33, 7, 1), (40, 9, 5), (63, 5, 2), (64, 36, 5), (65, 7, 1), (90, 9, 5), (96, 4, 2), (129, 3, 1)]
_temporal_cache = {}


def _temporal_case(dev, T, S, H, pre):
    """qkv [(b t), s, 3C] on the device and the fp64 result [(b t), s, C], computed once per case"""
    key = (T, S, H, pre)
    if key not in _temporal_cache:
        B, C = 2, 64 * H
        qkv = _rand((B * T, S, 3 * C), 11 + T)
        if pre:
            qkv[..., :C] *= QK_C
        qkv = qkv.half()
        x = qkv.view(B, T, S, 3, H, 64).permute(3, 0, 2, 4, 1, 5).double()  # [3, B, S, H, T, 64]
        logits = x[0] @ x[1].transpose(-1, -2) * (math.log(2.0) if pre else 0.125)
        ref = (torch.softmax(logits, -1) @ x[2]).permute(0, 3, 1, 2, 4).reshape(B * T, S, C)
        _temporal_cache[key] = (qkv.to(dev), ref)
    return _temporal_cache[key]


def _temporal_launch(qkv, T, S, H, pre):
    """the launch of `_engine`'s temporal regime; returns (output, guard rows before, guard rows after)"""
    from seva import ops
    B, C = 2, 64 * H
    buf = torch.full((B * T + 2 * GUARD, S, C), 7.0, device=qkv.device, dtype=torch.float16)
    out = buf[GUARD:GUARD + B * T]
    out.fill_(float("nan"))
    ops.attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], out, nb0=B, nb1=S, heads=H, lq=T, lk=T,
                  q_strides=(T * S * 3 * C, 3 * C, S * 3 * C), k_strides=(T * S * 3 * C, 3 * C, S * 3 * C),
                  o_strides=(T * S * C, C, S * C), q_prescaled=pre)
    torch.cuda.synchronize()
    return out, buf[:GUARD], buf[GUARD + B * T:]


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("T,S,H", TEMPORAL)
def test_attention_temporal_strided_33_to_129_frames(dev, T, S, H, pre):
    qkv, ref = _temporal_case(dev, T, S, H, pre)
    out, before, after = _temporal_launch(qkv, T, S, H, pre)
    assert torch.isfinite(out).all(), "an output row was not written"
    assert bool((before == 7.0).all()) and bool((after == 7.0).all()), "a row outside the output was written"
    err = rel_l2(out.cpu(), ref)
    print(f"\ntemporal attention T={T} S={S} H={H} {'pre-scaled' if pre else 'plain'}: rel-L2 vs fp64 {err:.3e}")
    assert err < 2e-3


def _dense_case(dev, L, pre):
    B, H = 3, 2
    C = 64 * H
    qkv = _rand((B, L, 3 * C), 40 + L)
    if pre:
        qkv[..., :C] *= QK_C
    qkv = qkv.half()
    x = qkv.view(B, L, 3, H, 64).permute(2, 0, 3, 1, 4).double()  # [3, B, H, L, 64]
    ref = (torch.softmax(x[0] @ x[1].transpose(-1, -2) * (math.log(2.0) if pre else 0.125), -1) @ x[2]).transpose(1, 2).reshape(B, L, C)
    return qkv.to(dev), ref, B, H, C


def _dense_launch(qkv, L, B, H, C, pre):
    from seva import ops
    out = torch.full((B, L, C), float("nan"), device=qkv.device, dtype=torch.float16)
    ops.attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], out, nb0=B, nb1=1, heads=H, lq=L, lk=L,
                  q_strides=(L * 3 * C, 0, 3 * C), k_strides=(L * 3 * C, 0, 3 * C), o_strides=(L * C, 0, C), q_prescaled=pre)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("L", [33, 64])
def test_attention_dense_layout_at_33_and_64_tokens(dev, L, pre):
    qkv, ref, B, H, C = _dense_case(dev, L, pre)
    out = _dense_launch(qkv, L, B, H, C, pre)
    assert torch.isfinite(out).all()
    assert rel_l2(out.cpu(), ref) < 2e-3


# ------------------------------------------------------------------------------------------------------------ b. route equality
@pytest.mark.parametrize("pre", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("T,S,H", [c for c in TEMPORAL if c[0] <= 64])
def test_two_wave_route_equals_four_wave_route_temporal(dev, T, S, H, pre, short2):
    """attn_kernel<2, 64> on one K/V buffer (knob 1) and attn_kernel<4, 64> on the ring (knob 0): equal bits, both correct."""
    qkv, ref = _temporal_case(dev, T, S, H, pre)
    outs = []
    for knob in (0, 1):
        short2(knob)
        out, before, after = _temporal_launch(qkv, T, S, H, pre)
        assert torch.isfinite(out).all() and bool((before == 7.0).all()) and bool((after == 7.0).all()), knob
        assert rel_l2(out.cpu(), ref) < 2e-3, knob
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("L", [33, 64])
def test_two_wave_route_equals_four_wave_route_dense(dev, L, pre, short2):
    qkv, ref, B, H, C = _dense_case(dev, L, pre)
    outs = []
    for knob in (0, 1):
        short2(knob)
        outs.append(_dense_launch(qkv, L, B, H, C, pre))
        assert rel_l2(outs[-1].cpu(), ref) < 2e-3, knob
    assert torch.equal(outs[0], outs[1])


def test_the_knob_does_not_reach_other_lengths(dev, short2):
    """lq <= 32, lq in 65 .. 128, and lk > 64 with lq <= 64 keep their kernels whatever the knob says (one K/V buffer holds one tile)."""
    from seva import ops
    B, H, C = 2, 1, 64
    for lq, lk in ((21, 21), (65, 65), (40, 70), (64, 200)):
        q, kv = _rand((B, lq, C), 60 + lq).half().to(dev), _rand((B, lk, 2 * C), 61 + lk).half().to(dev)
        outs = []
        for knob in (0, 1):
            short2(knob)
            out = torch.full((B, lq, C), float("nan"), device=dev, dtype=torch.float16)
            ops.attention(q, kv[..., :C], kv[..., C:], out, nb0=B, nb1=1, heads=H, lq=lq, lk=lk, q_strides=(lq * C, 0, C),
                          k_strides=(lk * 2 * C, 0, 2 * C), o_strides=(lq * C, 0, C))
            torch.cuda.synchronize()
            outs.append(out)
        ref = torch.softmax(q.double() @ kv[..., :C].double().transpose(-1, -2) * 0.125, -1) @ kv[..., C:].double()
        assert torch.equal(outs[0], outs[1]) and rel_l2(outs[1].cpu(), ref.cpu()) < 2e-3, (lq, lk)


# ------------------------------------------------------------------------------------------------------------ c. tiny width, layer-wise
def _wrapper_inputs(T, hw, seed, input_slots=(0,)):
    """Same recipe as oracle/make_goldens_semidense.py:semidense_inputs (x, t, cond [uncond; cond])."""
    from seva import synthetic as synth
    sc = synth.synth_scene(T, (hw, hw), tuple(input_slots), seed=seed)
    x = torch.randn(2 * T, 4, hw, hw, generator=torch.Generator().manual_seed(seed + 1))
    c = {k: torch.cat((sc["uc"][k], sc["cond"][k]), 0) for k in ("crossattn", "concat", "dense_vector")}
    t = torch.full((2 * T,), 979, dtype=torch.int64)
    return x, t, c


@pytest.mark.parametrize("T", [33, 41, 64, 65, 90])
def test_tiny_layers_at_long_windows(dev, T):
    """The tiny network (model_channels = 64) on an 8 x 8 latent, every layer against the CPU oracle: temporal attention with T
    tokens on both sides of 32 and of 64, joint attention over T * 64 .. T tokens."""
    from oracle import seva_ref as O
    from seva.model import SGMWrapper
    net, sd = _build("tiny", dev)  # a fresh engine: its arena holds this shape's buffers only (what _layer_table reads)
    eng = net.engine()
    x, t, c = _wrapper_inputs(T, 8, seed=1200 + T, input_slots=tuple(range(0, T, 5)))
    trace = {}
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ref = O.sgm_wrapper_forward(sd, x, t, c, T, trace=trace)
    y = SGMWrapper(net)(x.to(dev), t.to(dev), {k: v.to(dev) for k, v in c.items()}, num_frames=T)
    torch.cuda.synchronize()
    rows = _layer_table(eng, trace, x.shape[0])
    err = rel_l2(y.cpu(), ref)
    worst = sorted(rows, key=lambda r: -r[1])[:3]
    print(f"\ntiny T={T} 8x8: output rel-L2 {err:.3e}; {len(rows)} layers, worst " + ", ".join(f"{p} {e:.3e}" for p, e, _ in worst))
    assert len(rows) >= 40
    bad = [(p, e) for p, e, _ in rows if not e < LAYER_TOL]
    assert not bad, f"layers beyond tolerance: {bad[:5]}"
    assert err < NET_TOL


# ------------------------------------------------------------------------------------------------------------ d. full width
@pytest.fixture(scope="module")
def full(dev):
    return _build("full", dev)


@pytest.mark.parametrize("T", [41, 64, 65, 90])
def test_forward_vs_reference_at_long_windows(dev, full, T):
    """One SGMWrapper call of the 1.3B network, 16 x 16 latent, 32 input views in the slots the reference's plan gives them, against
    the reference's stored output (all 2T latents).  NET_TOL overall and per latent: the bound rests on the engine's default
    split-precision classes (profiles/semidense_parity.log)."""
    from seva.model import SGMWrapper
    g = load_golden(f"g15_T{T}_forward")
    ref, slots, seed, hw = g["y"], g["input_slots"].tolist(), int(g["seed"]), int(g["h"])
    assert (int(g["T"]), hw, int(g["w"])) == (T, 16, 16) and len(slots) == 32 and ref.shape == (2 * T, 4, hw, hw)
    net, _ = full
    x, t, c = _wrapper_inputs(T, hw, seed, slots)
    y = SGMWrapper(net)(x.to(dev), t.to(dev), {k: v.to(dev) for k, v in c.items()}, num_frames=T).cpu()
    assert y.shape == ref.shape and torch.isfinite(y).all()
    err = rel_l2(y, ref)
    per = [rel_l2(y[i], ref[i]) for i in range(2 * T)]
    print(f"\n1.3B forward T={T} {hw}x{hw} (B={2 * T}) vs REFERENCE on {2 * T} latents: rel-L2 {err:.3e}; per latent max {max(per):.3e} "
          f"(row {per.index(max(per))}) min {min(per):.3e}; max-abs {float((y - ref).abs().max()):.3e} "
          f"(|ref| max {float(ref.abs().max()):.2f})")
    assert err < NET_TOL and max(per) < NET_TOL


def test_bitwise_promises_at_41_views(dev, full):
    """T = 41, full width, 16 x 16: two eager forwards give equal bits, the hipGraph replay equals them, and the conditional half
    launched alone (batch T) is bitwise the conditional half of the CFG batch (2T) -- what the CFG split of the one long first-pass
    window over a pair of ranks relies on."""
    net, _ = full
    eng = net.engine()
    T = 41
    x, t, c = _wrapper_inputs(T, 16, 77, tuple(range(32)))
    x, concat, t, y, dense = [v.to(dev) for v in (x, c["concat"], t, c["crossattn"], c["dense_vector"])]
    a = eng.forward(x, concat, t, y, dense, T).clone()
    b = eng.forward(x, concat, t, y, dense, T).clone()
    assert torch.isfinite(a).all() and 1e-3 < float(a.abs().mean()) < 1e2
    assert torch.equal(a, b)
    assert torch.equal(a, eng.forward_graphed(x, concat, t, y, dense, T))
    hi = eng.forward(x[T:], concat[T:], t[T:], y[T:], dense[T:], T).clone()
    lo = eng.forward(x[:T], concat[:T], t[:T], y[:T], dense[:T], T).clone()
    assert torch.equal(hi, a[T:]), "conditional half alone differs from the conditional half of the CFG batch"
    assert torch.equal(lo, a[:T])


# ------------------------------------------------------------------------------------------------------------ e. the driver
def _scene(dev, n, n_in, hw):
    from seva import synthetic as synth
    g = torch.Generator().manual_seed(3)
    lat = (torch.randn(n_in, 4, hw, hw, generator=g) * 0.9).to(dev)
    tok = torch.randn(1024, generator=g)
    return synth.orbit_c2w(n), synth.default_K(n), lat, (tok / tok.norm()).to(dev)


def test_semidense_trajectory_on_gpu_tiny(dev):
    """12 inputs, 60 frames, `interp-gt`: one first-pass window of 21 views, second-pass windows of 33 (the inputs ride along), two
    steps each, tiny network.  Finite, deterministic, inputs untouched; a second-pass window re-run alone (as another rank would run it)
    reproduces its frames bit for bit, from the noise draw of ITS length at ITS place in the one CPU stream."""
    from seva import pipeline
    from seva.model import SGMWrapper
    net, _ = _build("tiny", dev)
    n, n_in, hw, steps = 60, 12, 8, 2
    c2ws, Ks, lat, tok = _scene(dev, n, n_in, hw)
    ids = list(range(n_in))
    wrap = SGMWrapper(net)
    kw = dict(clip_token=tok, T=21, num_steps=steps, device=dev, chunk_strategy="interp-gt", cfg=(3.0, 2.0), guider=(1, 2))
    with torch.no_grad():
        a = pipeline.run_trajectory(wrap, lat, c2ws, Ks, ids, **kw)
        b = pipeline.run_trajectory(wrap, lat, c2ws, Ks, ids, **kw)
    plan = a["plan"]
    assert (plan.T1, plan.T2) == (21, 33) and len(plan.pass1) == 1 and len(plan.pass2) >= 2
    assert [len(w.slot_frame) for w in plan.pass1 + plan.pass2] == [21] + [33] * len(plan.pass2)
    z = a["latents"]
    assert z.shape == (n, 4, hw, hw) and torch.isfinite(z).all()
    assert torch.equal(z, b["latents"])
    assert torch.equal(z[:n_in], lat)
    assert all(float(z[f].abs().max()) > 0 for f in range(n_in, n))
    win = plan.pass2[-1]
    latents_of = {**{i: lat[i] for i in ids}, **a["anchor_latents"]}
    g0 = torch.Generator().manual_seed(23)
    noises = [torch.randn((len(w.slot_frame), 4, hw, hw), generator=g0) for w in plan.pass1 + plan.pass2]
    with torch.no_grad():
        zz = pipeline.run_window(win, latents_of, wrap, c2ws, Ks, hw=(hw, hw), num_steps=steps, cfg=2.0, cfg_min=1.2, guider=2,
                                 camera_scale=2.0, noise=noises[win.global_index],
                                 step_seed=(23 * 1000003 + 7919 * (win.global_index + 1)) & 0x7FFFFFFFFFFF, clip_token=tok, device=dev)
    assert zz.shape[0] == 33
    for fid, slot in zip(win.target_ids, win.target_slots):
        assert torch.equal(zz[slot], z[fid])


def test_one_pass_window_of_90_views(dev):
    """The reference's `--T 90`: 32 inputs and 58 targets in ONE window through `run_views`, tiny network, two steps."""
    from seva import pipeline
    from seva.model import SGMWrapper
    net, _ = _build("tiny", dev)
    n, n_in, hw = 90, 32, 8
    c2ws, Ks, lat, tok = _scene(dev, n, n_in, hw)
    ids = list(range(n_in))
    with torch.no_grad():
        res = pipeline.run_views(SGMWrapper(net), lat, c2ws, Ks, ids, T=90, clip_token=tok, num_steps=2, device=dev)
    plan = res["plan"]
    assert len(plan.pass1) == 1 and not plan.pass2 and len(plan.pass1[0].slot_frame) == 90
    assert plan.pass1[0].target_ids == list(range(n_in, n))
    z = res["latents"]
    assert z.shape == (n, 4, hw, hw) and torch.isfinite(z).all() and torch.equal(z[:n_in], lat)
    assert all(float(z[f].abs().max()) > 0 for f in range(n_in, n))
