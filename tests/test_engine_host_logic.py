"""CPU checks of the host side of the product: module tree == reference state_dict contract,
weight packing layouts, engine orchestration (with tests/fake_ops.py standing in for the HIP
kernels), sampler host logic, C-ABI symbol export.  No GPU work happens here."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import fake_ops
from conftest import ROOT, load_golden, rel_l2


def _shapes(tag):
    g = load_golden(f"g0_keys_{tag}")
    return {str(k): tuple(int(s) for s in str(v).split(",")) for k, v in zip(g["keys"], g["shapes"])}


@pytest.mark.parametrize("tag", ["full", "tiny"])
def test_state_dict_contract(tag):
    """Same 1146 keys, shapes and order as the reference Seva (meta device, bf16, assign=True)."""
    from seva.model import Seva, SevaParams
    params = SevaParams() if tag == "full" else SevaParams(model_channels=64)
    with torch.device("meta"):
        net = Seva(params).to(torch.bfloat16)
    sd = net.state_dict()
    ref = _shapes(tag)
    assert list(sd.keys()) == list(ref.keys())
    assert {k: tuple(v.shape) for k, v in sd.items()} == ref
    assert all(v.dtype == torch.bfloat16 for v in sd.values())
    if tag == "full":
        assert len(sd) == 1146 and sum(v.numel() for v in sd.values()) == 1263968004
    fake = {k: torch.empty(s, dtype=torch.bfloat16, device="meta") for k, s in ref.items()}
    missing, unexpected = net.load_state_dict(fake, strict=False, assign=True)
    assert not missing and not unexpected


def test_layout_names_match_reference_regimes():
    from seva._arch import build_layout
    from seva.model import SevaParams
    lay = build_layout(SevaParams())
    mv = [s for s in lay.all_specs() if s.kind == "mvt"]
    assert len(mv) == 16 and sum(1 for s in lay.all_specs() if s.kind == "res") == 22
    joint = sorted(s.prefix for s in mv if s.joint)
    assert joint == sorted(["middle_block.1"] + [f"output_blocks.{i}.1" for i in (3, 4, 5, 6, 7, 8)])
    assert [s.heads for s in mv if s.prefix.startswith("input_blocks")] == [5, 5, 10, 10, 20, 20]


def test_weight_packing_layouts():
    from seva._engine import interleave_geglu, pack_conv3x3
    g = torch.Generator().manual_seed(0)
    w, b, a = torch.randn(512, 64, generator=g), torch.randn(512, generator=g), torch.randn(10, 64, generator=g)
    wi, bi = interleave_geglu(w, b)
    out = torch.empty(10, 256)
    fake_ops.gemm(a.half(), wi.half(), bias=bi, out_f32=out, geglu=True)
    y = a.half().float() @ w.half().float().T + b
    assert torch.allclose(out, y[:, :256] * F.gelu(y[:, 256:]), atol=1e-5)
    wc, x = torch.randn(32, 64, 3, 3, generator=g), torch.randn(2, 64, 5, 6, generator=g)
    o = torch.empty(2 * 5 * 6, 32)
    fake_ops.conv3x3(x.permute(0, 2, 3, 1).contiguous().half(), pack_conv3x3(wc), out_f32=o)
    ref = F.conv2d(x.half().float(), wc.half().float(), None, padding=1)
    assert torch.allclose(o.view(2, 5, 6, 32).permute(0, 3, 1, 2), ref, atol=1e-4)
    assert pack_conv3x3(torch.randn(8, 11, 3, 3), 64).shape == (8, 576)


def _cpu_engine(tag="tiny", precision=None):
    """Engine on CPU with the HIP ops replaced by fake_ops (test-only construction)."""
    from seva import _engine, synthetic as synth
    from seva.model import Seva, SevaParams
    params = SevaParams() if tag == "full" else SevaParams(model_channels=64)
    sd = synth.synth_state_dict(_shapes(tag))
    with torch.device("meta"):
        net = Seva(params)
    net.load_state_dict(sd, strict=True, assign=True)
    orig = _engine.SevaEngine.__dict__["_resolve_device"]
    _engine.SevaEngine._resolve_device = staticmethod(lambda m: torch.device("cpu"))  # test seam
    try:
        eng = _engine.SevaEngine(net, precision)
    finally:
        _engine.SevaEngine._resolve_device = orig
    return eng, sd


@pytest.fixture()
def patched(monkeypatch):
    from seva import _engine
    monkeypatch.setattr(_engine, "ops", fake_ops)
    monkeypatch.setattr(_engine, "require_cuda", lambda *a: None)


def test_engine_orchestration_vs_oracle(patched):
    from oracle import seva_ref as O
    eng, sd = _cpu_engine()
    g = load_golden("g3_tiny_forward")
    T = int(g["T"])
    y = eng.forward(g["x"], g["concat"], g["t"], g["crossattn"], g["dense_vector"], T)
    err = rel_l2(y, g["y"])
    trace = {}
    O.sgm_wrapper_forward(sd, g["x"], g["t"], {k: g[k] for k in ("crossattn", "concat", "dense_vector")}, T, trace=trace)
    worst = 0.0
    for key, t in eng.arena.bufs.items():
        if key[0].startswith("out:") and key[0][4:] in trace:
            ref = trace[key[0][4:]]
            got = t.view(ref.shape[0], ref.shape[2], ref.shape[3], ref.shape[1]).permute(0, 3, 1, 2)
            worst = max(worst, rel_l2(got, ref))
    print(f"emulated-kernel engine vs golden {err:.2e}; worst layer {worst:.2e}")
    assert err < 2e-3 and worst < 3e-3


@pytest.mark.parametrize("T,h,w,lc", [(3, 8, 24, 1), (2, 8, 8, 3)])
def test_engine_orchestration_odd_shapes(patched, T, h, w, lc):
    from oracle import seva_ref as O
    eng, sd = _cpu_engine()
    g = torch.Generator().manual_seed(T * 100 + h)
    n = 2 * T
    x, t = torch.randn(n, 11, h, w, generator=g), torch.randint(0, 1000, (n,), generator=g)
    y, dense = torch.randn(n, lc, 1024, generator=g), torch.randn(n, 6, h, w, generator=g)
    out = eng.forward(x, None, t, y, dense, T)
    assert rel_l2(out, O.seva_forward(sd, x, t, y, dense, T)) < 2e-3


def test_engine_groupnorm_statistics_from_producer_epilogues(patched, monkeypatch):
    """GroupNorm statistics emitted by the producing conv / GEMM epilogue (seva_gemm_desc.ch_stats) and consumed through
    seva_groupnorm_desc.stats1 / stats2: same network output as the separate statistics pass, including the decoder's
    two-source (skip concat) GroupNorms; the emulated groupnorm USES the buffers it is handed, so a stale or mismatched
    buffer would show as an O(1) error."""
    eng, _ = _cpu_engine()
    g = torch.Generator().manual_seed(29)
    T, h, w = 2, 32, 32
    n = 2 * T
    x, t = torch.randn(n, 11, h, w, generator=g), torch.randint(0, 1000, (n,), generator=g)
    y, dense = torch.randn(n, 1, 1024, generator=g), torch.randn(n, 6, h, w, generator=g)
    eng.gn_fused_stats = 0
    ref = eng.forward(x, None, t, y, dense, T).clone()
    calls = {"with": 0, "two_source": 0, "without": 0}
    real = fake_ops.groupnorm

    def counting(x1, x2, *a, **k):
        if k.get("stats1") is not None:
            calls["with"] += 1
            calls["two_source"] += k.get("stats2") is not None
        else:
            calls["without"] += 1
        return real(x1, x2, *a, **k)

    monkeypatch.setattr(fake_ops, "groupnorm", counting)
    eng.gn_fused_stats = 2  # wherever hw % 64 == 0 and c >= 128 (the default, 1, also asks for >= 320 tiles per launch)
    out = eng.forward(x, None, t, y, dense, T)
    err = rel_l2(out, ref)
    print(f"producer-epilogue statistics vs statistics pass: {err:.2e}; GroupNorms with / without: {calls}")
    assert calls["with"] >= 8 and calls["two_source"] >= 2 and calls["without"] >= 1
    # last-bit differences of the statistics re-roll f16 roundings downstream (as in the sliced-chain test below)
    assert err < 2e-3


@pytest.mark.parametrize("frames", [1, 2])
def test_engine_frame_sliced_chains_match_unsliced(patched, frames):
    """Frame-sliced execution of the LN -> GEMM -> ... chains (engine._slice_rows) is the same computation.  (Bitwise on
    the GPU, tests/test_model_gpu.py; the torch-CPU emulation picks GEMM / LayerNorm kernels by row count and the differences pass through f16 roundings, so this
    only guards against slicing the wrong rows, which would be an O(1) error.)"""
    eng, _ = _cpu_engine()
    g = torch.Generator().manual_seed(17)
    T, h, w = 3, 8, 16
    n = 2 * T
    x, t = torch.randn(n, 11, h, w, generator=g), torch.randint(0, 1000, (n,), generator=g)
    y, dense = torch.randn(n, 1, 1024, generator=g), torch.randn(n, 6, h, w, generator=g)
    eng.slice_frames = 0
    ref = eng.forward(x, None, t, y, dense, T).clone()
    eng.slice_frames, eng.slice_min_bytes, eng.slice_attn = frames, 0, True  # force slicing at every level
    out = eng.forward(x, None, t, y, dense, T)
    err = rel_l2(out, ref)
    print(f"sliced ({frames} frame) vs unsliced, emulated kernels: {err:.2e}")
    assert err < 2e-3


def test_sampler_host_logic_vs_golden(patched, monkeypatch):
    """Product sampler classes driven by the emulated kernels reproduce the reference loop."""
    from seva import sampling as S
    from seva import synthetic as synth
    monkeypatch.setattr(S, "ops", fake_ops)
    monkeypatch.setattr(S, "_need_gpu", lambda *a: None)
    eng, _ = _cpu_engine()
    g = load_golden("g7_loop_tiny")
    T, hw, steps = int(g["T"]), int(g["hw"]), int(g["steps"])
    sc = synth.synth_scene(T, (hw, hw), (0,), seed=int(g["scene_seed"]))
    disc = S.DDPMDiscretization()
    den = S.DiscreteDenoiser(disc, num_idx=1000, device="cpu")
    sampler = S.EulerEDMSampler(disc, S.MultiviewCFG(1.2), num_steps=steps, verbose=False, device="cpu")
    it = iter(list(g["eps"]))
    sampler.noise_fn = lambda x: next(it)
    net = lambda x, t, c, num_frames: eng.forward(x, c["concat"], t, c["crossattn"], c["dense_vector"], num_frames)
    out = sampler(lambda x, s, c: den(net, x, s, c, num_frames=T), sc["noise"].clone(), scale=2.0,
                  cond=sc["cond"], uc=sc["uc"], verbose=False, c2w=sc["c2w"], K=sc["K"],
                  input_frame_mask=sc["input_frame_mask"])
    assert rel_l2(out, g["y"]) < 4e-3
    # guiders / schedules against the reference goldens (pure host logic)
    gg = load_golden("g6_guiders")
    sig = torch.full((T,), 24.2054) + 1e-6
    args = (gg["c2w"], gg["K"], gg["mask"].bool())
    assert rel_l2(S.VanillaCFG()(gg["d"], sig, 2.0), gg["y0"]) < 1e-6
    assert rel_l2(S.MultiviewCFG(1.2)(gg["d"], sig, 2.0, *args), gg["y1"]) < 1e-6
    assert rel_l2(S.MultiviewTemporalCFG(T, 1.2)(gg["d"], sig, 2.0, *args), gg["y2"]) < 1e-6
    g1 = load_golden("g1_schedules")
    assert torch.equal(disc(50), g1["sig50"]) and torch.equal(disc(4), g1["sig4"])
    assert torch.equal(den.sigmas, g1["table"]) and torch.equal(den.sigma_to_idx(g1["sig50"][:-1]), g1["idx50"])
    with pytest.raises(ValueError):
        disc.get_sigmas(1001)
    with pytest.raises(ValueError):
        S.append_dims(torch.zeros(2, 2), 1)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "stable-virtual-camera_amd", "seva")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+\S*oracle", src, re.M), f
                assert "/root/reference" not in src, f


def test_hip_path_fails_loudly_on_cpu():
    from seva import ops, sampling as S
    from seva._native import SevaNativeError
    from seva.model import Seva, SevaParams
    net = Seva(SevaParams(model_channels=64))
    with pytest.raises(SevaNativeError):
        net(torch.zeros(2, 11, 8, 8), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 1, 1024),
            torch.zeros(2, 6, 8, 8), num_frames=2)
    with pytest.raises(SevaNativeError):
        ops.gemm(torch.zeros(4, 64, dtype=torch.float16), torch.zeros(4, 64, dtype=torch.float16),
                 out_f32=torch.zeros(4, 4))
    with pytest.raises(SevaNativeError):
        S.VanillaCFG()(torch.zeros(4, 4, 2, 2), torch.ones(2), 2.0)


def test_vae_decoder_orchestration_vs_restatement(monkeypatch):
    """VAE decode engine (emulated kernels) vs oracle/vae_ref.py.  Parity with diffusers is UNPINNED."""
    from oracle import vae_ref as V
    from seva import _vae_engine, synthetic as synth
    from seva.modules.autoencoder import VaeDecoderWeights
    monkeypatch.setattr(_vae_engine, "ops", fake_ops)
    monkeypatch.setattr(_vae_engine, "require_cuda", lambda *a: None)
    monkeypatch.setattr(_vae_engine.VaeDecoderEngine, "_resolve_device", staticmethod(lambda w: torch.device("cpu")))
    full = {k: tuple(v.shape) for k, v in VaeDecoderWeights().state_dict().items()}
    assert full == V.decoder_shapes()
    small = (64, 64, 128, 128)  # same topology, narrower: keeps the CPU test fast
    wts = VaeDecoderWeights(block_out=small)
    shapes = V.decoder_shapes(block_out=small)
    assert {k: tuple(v.shape) for k, v in wts.state_dict().items()} == shapes
    sd = synth.synth_state_dict(shapes, 3)
    wts.load_state_dict(sd)
    eng = _vae_engine.VaeDecoderEngine(wts)
    z = torch.randn(2, 4, 6, 6, generator=torch.Generator().manual_seed(0)) * 0.18215 * 4
    out = eng.decode(z, 0.18215)
    ref = V.vae_decode(sd, z)
    assert out.shape == (2, 3, 48, 48)
    err = rel_l2(out, ref)
    print(f"vae decode (emulated kernels) vs restatement: {err:.2e}")
    assert err < 3e-3


def test_vae_encoder_orchestration_vs_restatement(monkeypatch):
    """VAE encode engine (emulated kernels) vs oracle/vae_ref.py.  Parity with diffusers is UNPINNED."""
    from oracle import vae_ref as V
    from seva import _vae_engine, synthetic as synth
    from seva.modules.autoencoder import VaeWeights
    monkeypatch.setattr(_vae_engine, "ops", fake_ops)
    monkeypatch.setattr(_vae_engine, "require_cuda", lambda *a: None)
    monkeypatch.setattr(_vae_engine.VaeEncoderEngine, "_resolve_device", staticmethod(lambda w: torch.device("cpu")))
    full = {k: tuple(v.shape) for k, v in VaeWeights().state_dict().items()}
    assert full == {**V.decoder_shapes(), **V.encoder_shapes()}
    small = (64, 64, 128, 128)
    wts = VaeWeights(block_out=small)
    shapes = {**V.decoder_shapes(block_out=small), **V.encoder_shapes(block_out=small)}
    assert {k: tuple(v.shape) for k, v in wts.state_dict().items()} == shapes
    sd = synth.synth_state_dict(shapes, 5)
    wts.load_state_dict(sd)
    eng = _vae_engine.VaeEncoderEngine(wts)
    x = torch.rand(2, 3, 48, 64, generator=torch.Generator().manual_seed(0)) * 2 - 1
    out = eng.encode(x, 0.18215)
    ref = V.vae_encode(sd, x)
    assert out.shape == (2, 4, 6, 8)
    err = rel_l2(out, ref)
    print(f"vae encode (emulated kernels) vs restatement: {err:.2e}")
    assert err < 3e-3
    with pytest.raises(ValueError):
        eng.encode(torch.zeros(1, 3, 20, 16), 0.18215)


def _guider_oracle_scale(c2w, K, mask, scale=2.0, cfg_min=1.2):
    """Independent restatement of the reference rule (sampling.py:160-187) for the cache tests."""
    from oracle import sampling_ref as SR
    T = c2w.shape[0]
    d = torch.cat([torch.zeros(T, 1, 1, 1), torch.ones(T, 1, 1, 1)], 0)  # u = 0, c = 1  ->  result = scale per frame
    return SR.guide(d, scale, 1, cfg_min, c2w, K, mask, T).reshape(T)


def test_multiview_cfg_under_inference_mode_and_across_scenes(monkeypatch):
    """reference do_sample creates c2w / K / mask under torch.inference_mode() (eval.py:1242,1286-1290):
    the guider must not read `_version` there, and a second scene whose freshly allocated tensors reuse the first
    scene's addresses must not be served the first scene's cached per-frame scale."""
    from seva import sampling as S
    from seva import synthetic as synth
    monkeypatch.setattr(S, "ops", fake_ops)
    monkeypatch.setattr(S, "_need_gpu", lambda *a: None)
    T = 6
    base = synth.orbit_c2w(T)
    K = synth.default_K(T)
    guider = S.MultiviewCFG(1.2)
    d = torch.cat([torch.zeros(T, 4, 2, 2), torch.ones(T, 4, 2, 2)], 0)
    sig = torch.ones(T)
    with torch.inference_mode():
        for trial in range(4):
            # scene A: frame 0 is the input, frame 3 sits on the input pose; scene B: frame 2 is the input
            c2w = base.clone()
            mask = torch.zeros(T, dtype=torch.bool)
            if trial % 2 == 0:
                mask[0] = True
                c2w[3] = c2w[0]
            else:
                mask[2] = True
                c2w[5] = c2w[2]
            Kc = K.clone()
            for _ in range(3):  # several steps of one trajectory hit the cache
                got = guider(d, sig, 2.0, c2w, Kc, mask)[:, 0, 0, 0]
                want = _guider_oracle_scale(c2w.clone(), Kc.clone(), mask.clone())
                assert torch.allclose(got, want), (trial, got, want)
            ent = guider._rule_cache
            assert ent is not None and ent[0][1] is c2w
            del c2w, mask, Kc  # the allocator may hand the same storage to the next scene


def test_sampler_resets_guider_cache_per_trajectory(monkeypatch):
    from seva import sampling as S
    monkeypatch.setattr(S, "ops", fake_ops)
    monkeypatch.setattr(S, "_need_gpu", lambda *a: None)
    guider = S.MultiviewCFG(1.2)
    guider._rule_cache = (("stale",) * 4, torch.zeros(3))
    sampler = S.EulerEDMSampler(S.DDPMDiscretization(), guider, num_steps=3, device="cpu")
    sampler.prepare_sampling_loop(torch.zeros(3, 4, 2, 2), {}, {}, None)
    assert guider._rule_cache is None


def test_vae_loader_is_strict_and_maps_legacy_attention_names(tmp_path, monkeypatch):
    """no silent random-init VAE, no silently dropped keys; the published SD-2.1 VAE file's
    deprecated mid-block attention names (query/key/value/proj_attn, 1x1-conv shaped) must land in to_q/.../to_out.0."""
    import warnings

    import safetensors.torch
    from seva.modules import autoencoder as A
    monkeypatch.delenv("SEVA_VAE_PATH", raising=False)
    monkeypatch.delenv("SEVA_VAE_RANDOM_INIT", raising=False)
    with pytest.raises(RuntimeError, match="no VAE weights"):
        A.AutoEncoder(chunk_size=1)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        ae = A.AutoEncoder(chunk_size=1, random_init=True)
    assert ae.random_init and any("RANDOM-INIT" in str(x.message) for x in w)
    # a checkpoint in the legacy naming, attention projections stored as 1x1 convs
    g = torch.Generator().manual_seed(0)
    sd = {k: torch.randn(v.shape, generator=g) for k, v in ae.module.state_dict().items()}
    legacy = {}
    inv = {v: k for k, v in A._LEGACY_ATTN.items()}
    for k, v in sd.items():
        m = re.match(r"^((?:encoder|decoder)\.mid_block\.attentions\.0)\.(to_q|to_k|to_v|to_out\.0)\.(weight|bias)$", k)
        if m:
            k2 = f"{m.group(1)}.{inv[m.group(2)]}.{m.group(3)}"
            legacy[k2] = v[:, :, None, None].clone() if m.group(3) == "weight" else v
        else:
            legacy[k] = v
    assert any(".query." in k for k in legacy)
    path = str(tmp_path / "vae.safetensors")
    safetensors.torch.save_file(legacy, path)
    monkeypatch.setenv("SEVA_VAE_PATH", path)
    ae2 = A.AutoEncoder(chunk_size=1)
    assert not ae2.random_init
    for k, v in ae2.module.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # one key missing -> loud failure
    broken = dict(legacy)
    broken.pop("decoder.mid_block.attentions.0.query.weight")
    safetensors.torch.save_file(broken, path)
    with pytest.raises(RuntimeError, match="missing"):
        A.AutoEncoder(chunk_size=1)
    extra = dict(legacy)
    extra["decoder.something_else.weight"] = torch.zeros(3)
    safetensors.torch.save_file(extra, path)
    with pytest.raises(RuntimeError, match="unexpected"):
        A.AutoEncoder(chunk_size=1)



def test_fp8_engine_orchestration(patched):
    """BASELINE config 5 wiring on the CPU (emulated kernels): in fp8 mode every eligible layer (C % 128 == 0: QKV, GEGLU,
    FF2, ResBlock convs) gets e4m3 weights + scale bytes and the engine routes e4m3 activations to them; the result stays
    close to the fp32 oracle at e4m3 accuracy (a few per cent -- a separate accuracy class, never the parity mode)."""
    from oracle import seva_ref as O
    eng, sd = _cpu_engine(precision="fp8")
    assert eng.fp8
    q = [k for k in eng.W if k.endswith("8e")]
    assert any(".qkv8e" in k for k in q) and any(".w18e" in k for k in q) and any(".w28e" in k for k in q)
    assert any(".conv1.w8e" in k for k in q) and any(".conv2.w8e" in k for k in q)
    # the C = 64 level would need its reductions padded 64 -> 128 (2x): stays f16; C = 320-style paddings (<= 25 %) are taken
    assert not any(k.startswith("input_blocks.1.") and k.endswith("8e") for k in q)
    from seva._engine import _pad128
    assert (_pad128(320), _pad128(960), _pad128(640)) == (384, 1024, 640)
    T, h, w = 2, 8, 8
    g = torch.Generator().manual_seed(3)
    n = 2 * T
    x, t = torch.randn(n, 11, h, w, generator=g), torch.randint(0, 1000, (n,), generator=g)
    y, dense = torch.randn(n, 1, 1024, generator=g), torch.randn(n, 6, h, w, generator=g)
    out = eng.forward(x, None, t, y, dense, T)
    ref = O.seva_forward(sd, x, t, y, dense, T)
    err = rel_l2(out, ref)
    print(f"fp8 engine (emulated kernels) vs fp32 oracle: rel-L2 {err:.3e}")
    assert 1e-3 < err < 0.15
    f16_eng, _ = _cpu_engine()
    assert not f16_eng.fp8 and not any(k.endswith("8e") for k in f16_eng.W)


def test_clip_engine_orchestration_vs_restatement(monkeypatch):
    """CLIP conditioner host logic on the CPU (emulated kernels): weight packing incl. the GELU-through-GEGLU packing, the
    patch-embedding GEMM with the positional embedding as residual, token plumbing, pooling; strict open_clip loading."""
    from oracle import clip_ref as CR
    from seva import _clip_engine, synthetic as synth
    from seva.modules import conditioner as Cd
    monkeypatch.setattr(_clip_engine, "ops", fake_ops)
    monkeypatch.setattr(_clip_engine, "require_cuda", lambda *a: None)
    monkeypatch.setattr(_clip_engine.ClipEngine, "_resolve_device", staticmethod(lambda w: torch.device("cpu")))
    monkeypatch.delenv("SEVA_CLIP_PATH", raising=False)
    monkeypatch.delenv("SEVA_CLIP_RANDOM_INIT", raising=False)
    with pytest.raises(RuntimeError, match="no weights"):
        Cd.CLIPConditioner()
    p = Cd.ViTParams(width=320, layers=2, embed_dim=64)
    cond = Cd.CLIPConditioner(p, random_init=True)
    shapes = CR.vit_shapes(320, 2, 14, 224, 1280, 64)
    assert {k: tuple(v.shape) for k, v in cond.module.state_dict().items()} == shapes
    sd = synth.synth_state_dict(shapes, 5)
    g = torch.Generator().manual_seed(1)
    sd["visual.class_embedding"] = 0.02 * torch.randn(320, generator=g)
    sd["visual.positional_embedding"] = 0.02 * torch.randn(257, 320, generator=g)
    sd["visual.proj"] = torch.randn(320, 64, generator=g) * 320 ** -0.5
    for k in shapes:
        if k.endswith("in_proj_weight"):
            sd[k] = torch.randn(shapes[k], generator=g) * 320 ** -0.5
    # an open_clip CLIP checkpoint also carries the text tower: dropped knowingly; a missing vision key is an error
    full = dict(sd, **{"logit_scale": torch.zeros(()), "token_embedding.weight": torch.zeros(4, 4)})
    Cd.load_open_clip(cond.module, full)
    broken = {k: v for k, v in full.items() if k != "visual.ln_post.bias"}
    with pytest.raises(RuntimeError, match="missing"):
        Cd.load_open_clip(cond.module, broken)
    x = torch.rand(2, 3, 300, 260, generator=g) * 2 - 1
    got = cond(x)
    ref = CR.clip_conditioner(sd, x, heads=p.heads)
    err = rel_l2(got, ref)
    print(f"CLIP engine (emulated kernels) vs restatement: rel-L2 {err:.3e}")
    assert got.shape == (2, 64) and err < 2e-3
    assert rel_l2(cond.preprocess(x), CR.preprocess(x)) < 1e-3
