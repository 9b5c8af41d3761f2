"""Every engine switch and precision-mode combination on the device.

The kernels are pinned operator by operator elsewhere; this file pins the ENGINE under the switches `SevaEngine.__init__`, `_resample`
and `_VaeEngineBase.__init__` read -- the legs of every A/B timing and the user-facing opt-ins.  Machinery (environment handling,
call recorder, witnesses) is shared with tests/test_engine_switches_cpu.py, which runs the same configurations on emulated kernels.

Bounds, none looser than the class's existing one:
  * f16 configurations: rel-L2 < 1e-3 over the whole output (NET_TOL, BASELINE.json north_star), per latent too at full width;
  * fp8 configurations: 1e-3 < rel-L2 < 6e-2 and < 1e-1 per latent (tests/test_fp8_gpu.py; the lower bound witnesses e4m3 operands);
  * the two SEVA_FP8_PAD legs: finite and rel-L2 < 1e-1, an order-of-magnitude guard only (measured values: profiles/engine_switches.log);
  * VAE engines: rel-L2 < 2e-3 against oracle/vae_ref.py (tests/test_model_gpu.py).
References: the reference-generated goldens g3 / g4, else the fp32 CPU oracle, computed once per shape.

Inputs of the tiny network: (i) g3 (T=4, 16x16); (ii) the ragged (3, 8, 24) and (5, 16, 8); (iii) T=8, 32x32, n=16: levels of
1024 / 256 / 64 / 16 pixels, on both sides of the split-K limit (128 pixels), statistics-capable levels, joint attention of
8 * 256 = 2048 keys (>= ops.PV8_MIN_LQ); (iv) T=24, 32x32, n=24: joint attention of 24 * 256 = 6144 keys = ops.ATTN_SPLIT_MIN_LK, the
smallest 32x32 input whose joint level (1/2 resolution: the full-resolution level attends per frame) runs K/V-split -- the two
attention-split configurations have their witnesses here, and run on (iii) for the bound.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import rel_l2
from test_engine_switches_cpu import (check_folded_operands, env_name, golden_inputs, oracle_reference, random_inputs, report,
                                      summary, switched, witness_ff_unfused, witness_fold, witness_no_splitk, witness_stats)
from test_model_gpu import _build, _vae

NET_TOL = 1e-3               # tests/test_model_gpu.py
FP8_LO, FP8_HI, FP8_LATENT = 1e-3, 6e-2, 1e-1   # tests/test_fp8_gpu.py
FP8_PAD_GUARD = 1e-1
VAE_TOL = 2e-3               # tests/test_model_gpu.py::test_vae_*_vs_restatement


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from seva import _native
    _native.load()
    torch.set_num_threads(min(16, torch.get_num_threads()))  # the CPU oracles
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tiny(dev):
    return _build("tiny", dev)


@pytest.fixture(scope="module")
def full(dev):
    return _build("full", dev)


_PRECISION_ATTRS = ("_precision", "_attention", "_ff_precision", "_split")


def _net_is_default(net) -> bool:
    return net._engine is None and not any(a in net.__dict__ for a in _PRECISION_ATTRS)


def _run(monkeypatch, dev, net, env, inputs, precision="f16", inspect=None, **opts):
    """One configuration of `net` on `inputs`: (output on the CPU, recording, what `inspect(engine, recording)` returned)."""
    from seva import ops
    assert _net_is_default(net), "an earlier test leaked a non-default engine"

    def build():
        net.set_precision(precision, **opts)  # the switches are read when the engine is constructed
        return net.engine()

    def drop():
        for a in _PRECISION_ATTRS:
            net.__dict__.pop(a, None)
        net._engine = None

    with switched(monkeypatch, ops, env, build, drop) as (eng, rec):
        x, concat, t, y, dense, T = inputs
        args = [None if v is None else v.to(dev) for v in (x, concat, t, y, dense)]
        out = eng.forward(*args, T).cpu()  # the eager launch sequence: one pass, one recording
        ops.check_handoffs()
        seen = None if inspect is None else inspect(eng, rec)
        del eng
    assert _net_is_default(net)
    return out, rec, seen


# ------------------------------------------------------------------------------------------------------------------ tiny inputs
# key -> (T, h, w, n); the second tuple: (a level of more than 128 pixels with a channel-changing ResBlock, a level that only
# SEVA_GN_FUSED_STATS=2 takes: hw % 64 == 0 with c >= 128 and fewer than 16 tiles per sample)
TINY_INPUTS = {
    "g3": (None, (True, True)),                       # 256 pixels x 64 ch (128 -> 64 ResBlocks), 64 pixels x 128 ch
    "T3_8x24": ((3, 8, 24, None), (True, False)),     # 192 / 48 / 12 / 3 pixels
    "T5_16x8": ((5, 16, 8, None), (False, False)),    # 128 / 32 / 8 / 2 pixels: no level above the split-K limit
    "T8_32x32": ((8, 32, 32, 16), (True, True)),      # 1024 / 256 / 64 / 16 pixels
    "T24_32x32": ((24, 32, 32, 24), (True, True)),    # one scene of 24 frames: joint key length 6144
}
ALL_TINY = ["g3", "T3_8x24", "T5_16x8", "T8_32x32"]


def _tiny_case(key, sd):
    shape = TINY_INPUTS[key][0]
    if shape is None:
        return golden_inputs("g3_tiny_forward")
    inputs = random_inputs(*shape)
    return inputs, oracle_reference(sd, key, inputs)


_DEFAULTS: dict = {}


def _default(monkeypatch, dev, tag, net, key, inputs):
    """Recording and output of the default f16 engine on an input (once per input)."""
    if (tag, key) not in _DEFAULTS:
        out, rec, _ = _run(monkeypatch, dev, net, {}, inputs)
        _DEFAULTS[tag, key] = (out, summary(rec), rec)
    return _DEFAULTS[tag, key]


def _per_latent(out, ref):
    return max(rel_l2(out[i], ref[i]) for i in range(out.shape[0]))


# ================================================================================================================ A. tiny, f16
@pytest.mark.parametrize("key", ALL_TINY + ["T24_32x32"])
def test_tiny_default(dev, tiny, monkeypatch, key):
    """The other leg of every comparison below: the default engine fuses the feed-forwards, hands split-K workspaces to its convs,
    folds nothing, and gives the joint attention a K/V-split workspace exactly from ops.ATTN_SPLIT_MIN_LK keys."""
    from seva import ops
    net, sd = tiny
    inputs, ref = _tiny_case(key, sd)
    out, s, rec = _default(monkeypatch, dev, "tiny", net, key, inputs)
    err = rel_l2(out, ref)
    split = [c for c in rec.named("attention") if c.given("split_ws")]
    report("default", key, err, f"ff_fused {s['ff_fused']}, gemm {s['gemm']}, splitk_ws {s['splitk_ws']}, stats1 {s['gn_stats']}, "
                                f"split attention {len(split)}")
    assert s["ff_fused"] > 0 and s["splitk_ws"] > 0 and s["a2"] == 0 and rec.count("ff_fused_fp8") == 0
    assert all(c.kw["lk"] >= ops.ATTN_SPLIT_MIN_LK for c in split)
    assert (len(split) > 0) == (key == "T24_32x32")
    assert err < NET_TOL


TINY_ENV_CONFIGS = [
    ({"SEVA_FF_FUSED": 0}, "ff"),
    ({"SEVA_GN_FUSED_STATS": 0}, "stats0"),
    ({"SEVA_GN_FUSED_STATS": 2}, "stats2"),
    ({"SEVA_CONV_SPLITK": 0}, "splitk"),
    ({"SEVA_FOLD_SKIP": 1}, "fold"),
    ({"SEVA_FOLD_SKIP": 1, "SEVA_CONV_SPLITK": 0}, "fold_all"),
    ({"SEVA_FOLD_SKIP": 1, "SEVA_SPLIT_PRECISION": "skip"}, "fold_split"),
]


@pytest.mark.parametrize("key", ALL_TINY)
@pytest.mark.parametrize("env,kind", TINY_ENV_CONFIGS, ids=[env_name(e) for e, _ in TINY_ENV_CONFIGS])
def test_tiny_env_switch(dev, tiny, monkeypatch, env, kind, key):
    net, sd = tiny
    inputs, ref = _tiny_case(key, sd)
    _, d, _ = _default(monkeypatch, dev, "tiny", net, key, inputs)
    some_fold, more_stats = TINY_INPUTS[key][1]

    def inspect(eng, rec):
        check_folded_operands(rec, eng)
        return eng.gn_fused_stats

    out, rec, gn_mode = _run(monkeypatch, dev, net, env, inputs, inspect=inspect)
    s = summary(rec)
    if kind == "ff":
        wit = witness_ff_unfused(s, d)
    elif kind in ("stats0", "stats2"):
        mode = 0 if kind == "stats0" else 2
        assert gn_mode == mode
        wit = witness_stats(s, d, mode, more_stats)
    elif kind == "splitk":
        wit = witness_no_splitk(s, d)
    elif kind == "fold":
        wit = witness_fold(s, d, False, some_fold)
    elif kind == "fold_all":
        wit = witness_fold(s, d, True, some_fold) + "; " + witness_no_splitk(s, d)
    else:
        # SEVA_SPLIT_PRECISION=skip: every channel-changing ResBlock's raw input travels as [hi | lo], so every folded operand is
        # 2 cin wide (check_folded_operands ties each a2 to the split_raw GroupNorm that wrote it)
        wit = witness_fold(s, d, False, some_fold)
        n_split = rec.count("groupnorm", lambda c: c.given("split_raw"))
        assert n_split == s["changing"]
        wit += f"; split_raw on {n_split} of {s['changing']}"
    err = rel_l2(out, ref)
    report(env_name(env), key, err, wit)
    assert err < NET_TOL


def _split_events(rec) -> dict:
    """Calls that only a split-precision operand class makes."""
    gn = rec.named("groupnorm")
    return {
        "stem": rec.count("nchw_to_nhwc_f16", lambda c: c.given("split")),
        "raw": sum(c.given("split_raw") for c in gn),
        "gn_act": sum(c.given("split_out") and c.given("silu") for c in gn),       # ResBlock / head GroupNorms (SiLU)
        "gn_mvt": sum(c.given("split_out") and not c.given("silu") for c in gn),   # the transformers' input GroupNorm
        "ln": rec.count("layernorm_split"),
        "gemm_out": rec.count("gemm_split_out"),
        "geglu_out": rec.count("gemm_split_out", lambda c: c.given("geglu")),
        "cast": rec.count("cast_concat_f16_split"),
    }


SPLIT_TOKENS_AND_NONE = ("stem", "head", "skip", "skip_deep", "conv", "resample", "proj_in", "proj_out", "qkv", "ff", "none")


@pytest.mark.parametrize("key", ALL_TINY)
@pytest.mark.parametrize("token", SPLIT_TOKENS_AND_NONE)
def test_tiny_split_token_alone(dev, tiny, monkeypatch, token, key):
    """`set_precision("f16", split=token)`: exactly the producers of that operand class write [hi | lo], nothing else does."""
    from seva._engine import parse_split
    net, sd = tiny
    inputs, ref = _tiny_case(key, sd)
    out, rec, split = _run(monkeypatch, dev, net, {}, inputs, split=token, inspect=lambda eng, rec: set(eng.split))
    gn = rec.named("groupnorm")
    n_res = sum(c.given("dense") for c in gn)          # ResBlocks: their first GroupNorm takes the dense modulation
    n_mvt = sum(not c.given("silu") for c in gn)       # transformers
    n_changing = sum(c.given("raw_f16") for c in gn)
    assert n_res > 0 and n_mvt > 0 and n_changing > 0
    ev = _split_events(rec)
    want = dict.fromkeys(ev, 0)
    if token == "stem":
        want["stem"] = 1
    elif token == "head":
        want["gn_act"] = 1
    elif token == "skip":
        want["raw"] = n_changing
    elif token == "skip_deep":
        want["raw"] = ev["raw"]
        assert 0 < ev["raw"] < n_changing  # the ResBlocks below the top level only (cout >= 2 model_channels)
    elif token == "conv":
        want["gn_act"] = 2 * n_res
    elif token == "resample":
        want["cast"] = ev["cast"]
        assert ev["cast"] == sum(c.given("stride") or c.given("upsample") for c in rec.named("conv3x3")) > 0
    elif token == "proj_in":
        want["gn_mvt"] = n_mvt
    elif token == "proj_out":
        want["gemm_out"] = n_mvt  # the last FF2 of each transformer writes proj_out's operand; that feed-forward is not fused
        assert rec.count("ff_fused") > 0
    elif token == "qkv":
        want["ln"] = ev["ln"]
        assert ev["ln"] == rec.count("gemm", lambda c: c.given("col_scale_n")) > 0  # one split LayerNorm per QKV projection
    elif token == "ff":
        want["ln"], want["gemm_out"], want["geglu_out"] = ev["ln"], ev["gemm_out"], ev["geglu_out"]
        assert ev["ln"] == ev["gemm_out"] == ev["geglu_out"] > 0 and rec.count("ff_fused") == 0
    assert ev == want, (token, ev, want)
    assert split == parse_split(token)
    err = rel_l2(out, ref)
    report(f"split={token}", key, err, ", ".join(f"{k} {v}" for k, v in ev.items() if v) or "no split producer")
    assert err < NET_TOL


@pytest.mark.parametrize("key", ["T8_32x32", "T24_32x32"])
def test_tiny_attention_never_split(dev, tiny, monkeypatch, key):
    """SEVA_ATTN_SPLIT_KV=0: no attention gets a K/V-split workspace (the default gives one from 6144 keys: input (iv))."""
    net, sd = tiny
    inputs, ref = _tiny_case(key, sd)
    ref_out, _, d_rec = _default(monkeypatch, dev, "tiny", net, key, inputs)
    out, rec, _ = _run(monkeypatch, dev, net, {"SEVA_ATTN_SPLIT_KV": 0}, inputs)
    was = sum(c.given("split_ws") for c in d_rec.named("attention"))
    now = sum(c.given("split_ws") for c in rec.named("attention"))
    assert now == 0 and (was > 0) == (key == "T24_32x32")
    if was:
        assert not torch.equal(out, ref_out)  # one pass over the keys instead of two combined partial results: other roundings
    err = rel_l2(out, ref)
    report("ATTN_SPLIT_KV=0", key, err, f"attention with split_ws {was} -> 0")
    assert err < NET_TOL


@pytest.mark.parametrize("key", ["T8_32x32", "T24_32x32"])
def test_tiny_attention_split_three_ways(dev, tiny, monkeypatch, knobs, key):
    """SEVA_ATTN_SPLIT=3 sizes the workspace for three partial results, the library knob attn_split=3 makes the kernel use them."""
    from seva import ops
    net, sd = tiny
    inputs, ref = _tiny_case(key, sd)
    ref_out, _, d_rec = _default(monkeypatch, dev, "tiny", net, key, inputs)
    knobs(attn_split=3)
    out, rec, _ = _run(monkeypatch, dev, net, {"SEVA_ATTN_SPLIT": 3}, inputs)
    split = [c for c in rec.named("attention") if c.given("split_ws")]
    d_split = [c for c in d_rec.named("attention") if c.given("split_ws")]
    assert len(split) == len(d_split) and (len(split) > 0) == (key == "T24_32x32")
    for c, c0 in zip(split, d_split):
        k = c.kw
        assert k["lk"] >= ops.ATTN_SPLIT_MIN_LK
        assert k["split_ws"].shape[0] == ops.attention_split_workspace_numel(k["nb0"], k["heads"], k["lq"], 3)
        assert 2 * k["split_ws"].shape[0] == 3 * c0.kw["split_ws"].shape[0]
    if split:
        assert not torch.equal(out, ref_out)  # three partial results combine to other roundings than two: the knob reached the kernel
    err = rel_l2(out, ref)
    report("ATTN_SPLIT=3 + knob attn_split=3", key, err, f"{len(split)} attention calls with a 3-slot split_ws")
    assert err < NET_TOL


def test_tiny_folded_path_is_batch_invariant(dev, tiny, monkeypatch):
    """SEVA_FOLD_SKIP=1 + SEVA_CONV_SPLITK=0: frame 0 of a T = 2 call, alone (n = 2) and with a second scene behind it (n = 4): the
    same bits (the form of tests/test_split_operands_gpu.py::test_batch_invariance_under_all)."""
    net, _ = tiny
    g = torch.Generator().manual_seed(41)
    T, h, w, n = 2, 16, 16, 4
    x, t = torch.randn(n, 11, h, w, generator=g), torch.randint(0, 1000, (n,), generator=g)
    y, dense = torch.randn(n, 1, 1024, generator=g), torch.randn(n, 6, h, w, generator=g)
    env = {"SEVA_FOLD_SKIP": 1, "SEVA_CONV_SPLITK": 0}
    big, rec, _ = _run(monkeypatch, dev, net, env, (x, None, t, y, dense, T))
    small, rec2, _ = _run(monkeypatch, dev, net, env, (x[:2].contiguous(), None, t[:2].contiguous(), y[:2].contiguous(),
                                                        dense[:2].contiguous(), T))
    for r in (rec, rec2):
        s = summary(r)
        assert s["a2"] == s["changing"] > 0 and s["splitk_ws"] == 0
    assert torch.isfinite(big).all() and torch.equal(small[0], big[0]) and torch.equal(small, big[:2])


# ================================================================================================================ B. tiny, fp8
def _check_fp8(out, ref):
    err, worst = rel_l2(out, ref), _per_latent(out, ref)
    return err, worst, bool(torch.isfinite(out).all()) and FP8_LO < err < FP8_HI and worst < FP8_LATENT


@pytest.mark.parametrize("key", ["g3", "T8_32x32"])
@pytest.mark.parametrize("ff", ["f16", "fp8"])
@pytest.mark.parametrize("attention", ["f16", "fp8"])
def test_tiny_fp8_combinations(dev, tiny, monkeypatch, attention, ff, key):
    from seva import ops
    net, sd = tiny
    inputs, ref = _tiny_case(key, sd)
    out, rec, _ = _run(monkeypatch, dev, net, {}, inputs, precision="fp8", attention=attention, ff=ff)
    n_pv8, n_qv, n_ff8 = rec.count("attention_pv8"), rec.count("quantize_v_fp8"), rec.count("ff_fused_fp8")
    n_q8 = rec.count("gemm", lambda c: c.given("w_exp")) + rec.count("conv3x3", lambda c: c.given("w_exp"))
    assert n_q8 > 0
    # joint attention of T hw = 2048 keys on (iii), 256 on (i): the e4m3 P.V kernel takes the launches from ops.PV8_MIN_LQ
    assert n_pv8 == n_qv and (n_pv8 > 0) == (attention == "fp8" and key == "T8_32x32")
    assert all(c.kw["lq"] >= ops.PV8_MIN_LQ for c in rec.named("attention_pv8"))
    assert all(c.kw["lq"] < ops.PV8_MIN_LQ for c in rec.named("attention")) or attention == "f16"
    assert (n_ff8 > 0) == (ff == "fp8")
    if ff == "fp8":  # the feed-forwards the fused f16 kernel would run in fp8 mode: all of them moved
        assert rec.count("ff_fused") == 0
    err, worst, ok = _check_fp8(out, ref)
    report(f"fp8 attention={attention} ff={ff}", key, err, f"worst latent {worst:.3e}; e4m3 GEMM/conv {n_q8}, attention_pv8 {n_pv8}, "
                                                         f"ff_fused_fp8 {n_ff8}")
    assert ok, (err, worst)


@pytest.mark.parametrize("key", ["g3", "T8_32x32"])
def test_tiny_fp8_ff_unfused(dev, tiny, monkeypatch, key):
    """precision fp8, ff="fp8", SEVA_FF_FUSED=0: `_ff_fused_fp8` declines, no feed-forward is fused in either format; the widths that
    are multiples of 128 run the e4m3 two-kernel chain, C = 64 the f16 two-kernel path."""
    net, sd = tiny
    inputs, ref = _tiny_case(key, sd)
    out, rec, _ = _run(monkeypatch, dev, net, {"SEVA_FF_FUSED": 0}, inputs, precision="fp8", ff="fp8")
    geglu = rec.named("gemm")
    n8 = sum(c.given("geglu") and c.given("w_exp") for c in geglu)
    n16 = sum(c.given("geglu") and not c.given("w_exp") for c in geglu)
    assert rec.count("ff_fused_fp8") == 0 and rec.count("ff_fused") == 0 and n8 > 0 and n16 > 0
    err, worst, ok = _check_fp8(out, ref)
    report("fp8 ff=fp8 FF_FUSED=0", key, err, f"worst latent {worst:.3e}; ff_fused_fp8 0, GEGLU GEMMs e4m3 {n8} / f16 {n16}")
    assert ok, (err, worst)


# ================================================================================================================ C. full width
def _g4():
    return golden_inputs("g4_full_forward")


def test_full_default(dev, full, monkeypatch):
    net, _ = full
    inputs, ref = _g4()
    out, s, rec = _default(monkeypatch, dev, "full", net, "g4", inputs)
    err, worst = rel_l2(out, ref), _per_latent(out, ref)
    n_ph = rec.count("conv3x3_up_phases")
    report("default (1.3 B)", "g4", err, f"worst latent {worst:.3e}; ff_fused {s['ff_fused']}, gemm {s['gemm']}, splitk_ws "
                                         f"{s['splitk_ws']}, stats1 {s['gn_stats']}, up_phases {n_ph}")
    assert s["ff_fused"] > 0 and s["gn_stats"] > 0 and n_ph > 0 and s["a2"] == 0
    assert err < NET_TOL and worst < NET_TOL


FULL_ENV_CONFIGS = [
    ({"SEVA_FF_FUSED": 0}, "ff"),
    ({"SEVA_FOLD_SKIP": 1}, "fold"),
    ({"SEVA_UPSAMPLE_PHASES": 0}, "taps"),
    ({"SEVA_GN_FUSED_STATS": 0}, "stats0"),
    ({"SEVA_GN_FUSED_STATS": 2}, "stats2"),
    ({"SEVA_CONV_SPLITK": 0}, "splitk"),
]


@pytest.mark.parametrize("env,kind", FULL_ENV_CONFIGS, ids=[env_name(e) for e, _ in FULL_ENV_CONFIGS])
def test_full_env_switch(dev, full, monkeypatch, env, kind):
    net, _ = full
    inputs, ref = _g4()
    _, d, d_rec = _default(monkeypatch, dev, "full", net, "g4", inputs)

    out, rec, (mc, folds) = _run(monkeypatch, dev, net, env, inputs,
                                 inspect=lambda eng, rec: (eng.p.model_channels, check_folded_operands(rec, eng)))
    s = summary(rec)
    if kind == "ff":
        wit = witness_ff_unfused(s, d)
        assert rec.count("gemm", lambda c: c.given("geglu") and c.args[0].shape[1] == mc) > 0  # the C = 320 feed-forward as two kernels
    elif kind == "fold":
        # g4: levels of 1024 and 256 pixels fold, 64 and 16 keep the split-K convs
        wit = witness_fold(s, d, False, True)
        # under the default skip_deep the folded operand of a cout >= 640 ResBlock is [hi | lo], 2 cin columns against
        # [w_conv2 | w_skip | w_skip]; the top level's (cout = 320) stays plain
        deep = [f for f in folds if f["cout"] >= 2 * mc]
        assert deep and len(deep) < len(folds)
        assert all(f["split"] == (f["cout"] >= 2 * mc) and f["k2"] == (2 if f["split"] else 1) * f["cin"] for f in folds), folds
        wit += f"; {len(deep)} of them with a [hi | lo] operand of 2 cin columns"
    elif kind == "taps":
        n0, n1 = d_rec.count("conv3x3_up_phases"), rec.count("conv3x3_up_phases")
        up0, up1 = (r.count("conv3x3", lambda c: c.given("upsample")) for r in (d_rec, rec))
        assert n0 > 0 and up0 == 0 and n1 == 0 and up1 == n0
        assert s["ch_stats"] > d["ch_stats"]  # the nine-tap conv emits the statistics the phase convs leave to the GroupNorm
        wit = f"up_phases {n0} -> 0, conv3x3(upsample) 0 -> {up1}, ch_stats {d['ch_stats']} -> {s['ch_stats']}"
    elif kind in ("stats0", "stats2"):
        wit = witness_stats(s, d, 0 if kind == "stats0" else 2, True)  # 256 pixels x 640 channels: 8 tiles, mode 2 only
    else:
        wit = witness_no_splitk(s, d)
    err, worst = rel_l2(out, ref), _per_latent(out, ref)
    report(env_name(env) + " (1.3 B)", "g4", err, f"worst latent {worst:.3e}; {wit}")
    assert err < NET_TOL and worst < NET_TOL


def test_full_fp8_attention_and_ff(dev, full, monkeypatch):
    net, _ = full
    inputs, ref = _g4()
    out, rec, _ = _run(monkeypatch, dev, net, {}, inputs, precision="fp8", attention="fp8", ff="fp8")
    n_ff8, n_pv8 = rec.count("ff_fused_fp8"), rec.count("attention_pv8")
    # g4's attention launches stay below ops.PV8_MIN_LQ (1024 keys at most): the option is on, the e4m3 P.V kernel has nothing to take
    assert n_ff8 > 0 and rec.count("ff_fused") == 0 and n_pv8 == rec.count("quantize_v_fp8") == 0
    err, worst, ok = _check_fp8(out, ref)
    report("fp8 attention=fp8 ff=fp8 (1.3 B)", "g4", err, f"worst latent {worst:.3e}; ff_fused_fp8 {n_ff8}, attention_pv8 {n_pv8}")
    assert ok, (err, worst)


@pytest.mark.parametrize("ff", ["f16", "fp8"])
def test_full_fp8_pad(dev, full, monkeypatch, ff):
    """SEVA_FP8_PAD=1: reductions of 320 and 960 zero-padded to 384 and 1024.  With ff="fp8" the C = 320 feed-forwards go to
    seva_ff_fused_fp8, not to the padded chain (the precedence `_ff_fused_fp8` states)."""
    U8 = torch.uint8
    net, _ = full
    inputs, ref = _g4()
    out, rec, _ = _run(monkeypatch, dev, net, {"SEVA_FP8_PAD": 1}, inputs, precision="fp8", ff=ff)
    g8 = [c for c in rec.named("gemm") if c.given("w_exp")]
    c8 = [c for c in rec.named("conv3x3") if c.given("w_exp")]
    k_gemm, k_conv = {c.args[0].shape[1] for c in g8}, {c.args[0].shape[-1] for c in c8}
    assert 384 in k_gemm and 1024 in k_conv, (k_gemm, k_conv)  # (the network's only 960-deep reductions are ResBlock convs)
    assert rec.count("layernorm", lambda c: c.args[3].dtype == U8 and c.args[3].shape[1] == 384) > 0
    assert rec.count("groupnorm", lambda c: c.given("out_f8") and c.kw["out_f8"].shape[-1] == 1024) > 0
    padded_geglu = sum(c.given("geglu") and c.args[0].shape[1] == 384 for c in g8)
    n_ff8 = rec.count("ff_fused_fp8")
    if ff == "fp8":
        assert n_ff8 > 0 and padded_geglu == 0 and all(c.args[3].shape[0] == 8 * 320 for c in rec.named("ff_fused_fp8"))
    else:
        assert n_ff8 == 0 and padded_geglu > 0
    assert rec.count("ff_fused") == 0
    err, worst = rel_l2(out, ref), _per_latent(out, ref)
    report(f"fp8 FP8_PAD=1 ff={ff} (1.3 B)", "g4", err, f"worst latent {worst:.3e}; e4m3 GEMM K {sorted(k_gemm)}, conv cin "
                                                        f"{sorted(k_conv)}, padded GEGLU {padded_geglu}, ff_fused_fp8 {n_ff8}")
    assert torch.isfinite(out).all() and err < FP8_PAD_GUARD


# ================================================================================================================ D. VAE engines
VAE_DECODE = {"narrow": ((64, 64, 128, 128), 2, 6, 6), "wide": ((128, 256, 512, 512), 1, 16, 16)}
VAE_ENCODE = {"narrow": ((64, 64, 128, 128), 2, 48, 64), "wide": ((128, 256, 512, 512), 1, 128, 128)}
# a level that only SEVA_GN_FUSED_STATS=2 takes (hw % 64 == 0, c >= 128, fewer than 16 tiles per sample)?  Every case has one.  Narrow
# decoder: the 128-channel upsample conv that writes 576 pixels; wide decoder: 256 pixels x 512 channels; narrow encoder: 768 and
# 192 pixels x 128 channels; wide encoder: 256 pixels x 512 channels.
VAE_MORE_STATS = {("decode", "narrow"): True, ("decode", "wide"): True, ("encode", "narrow"): True, ("encode", "wide"): True}
_VAE_REF: dict = {}
_VAE_DEFAULT: dict = {}

VAE_CONFIGS = [({}, "default"), ({"SEVA_VAE_FOLD_SHORTCUT": 0}, "unfold"), ({"SEVA_GN_FUSED_STATS": 0}, "stats0"),
               ({"SEVA_GN_FUSED_STATS": 2}, "stats2")]


def _vae_run(monkeypatch, dev, env, side, width):
    """Decode / encode under `env`; the AutoEncoder is built inside (its engines read the environment at construction)."""
    from oracle import vae_ref as V
    from seva import ops
    block_out, n, h, w = (VAE_DECODE if side == "decode" else VAE_ENCODE)[width]
    box = {}

    def build():
        box["ae"], box["sd"] = _vae(dev, block_out)
        return box["ae"]

    with switched(monkeypatch, ops, env, build, box.clear) as (ae, rec):
        if side == "decode":
            x = torch.randn(n, 4, h, w, generator=torch.Generator().manual_seed(1)) * 0.18215 * 4
            out = ae.decode(x.to(dev)).cpu()
            eng = ae.engine()
        else:
            x = torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(4)) * 2 - 1
            out = ae.encode(x.to(dev)).cpu()
            eng = ae.encoder_engine()
        if (side, width) not in _VAE_REF:
            _VAE_REF[side, width] = (V.vae_decode if side == "decode" else V.vae_encode)(box["sd"], x)
        shortcut = {v.data_ptr() for k, v in eng.W.items() if k.endswith(".conv_shortcut.w")}
        folded = {v.data_ptr() for k, v in eng.W.items() if k.endswith(".conv2.wf")}
        assert shortcut and len(folded) == len(shortcut)
        s = summary(rec)
        s["shortcut_gemm"] = rec.count("gemm", lambda c: c.args[1].ptr in shortcut)
        s["a2_on_wf"] = rec.count("conv3x3", lambda c: c.given("a2") and c.args[1].ptr in folded)
        s["mode"], s["fold"] = eng.gn_fused_stats, eng.fold_shortcut
        del eng, ae
    return rel_l2(out, _VAE_REF[side, width]), s


@pytest.mark.parametrize("width", ["narrow", "wide"])
@pytest.mark.parametrize("side", ["decode", "encode"])
@pytest.mark.parametrize("env,kind", VAE_CONFIGS, ids=[env_name(e) for e, _ in VAE_CONFIGS])
def test_vae_switch(dev, monkeypatch, env, kind, side, width):
    if (side, width) not in _VAE_DEFAULT:
        _VAE_DEFAULT[side, width] = _vae_run(monkeypatch, dev, {}, side, width)
    err, s = _VAE_DEFAULT[side, width] if kind == "default" else _vae_run(monkeypatch, dev, env, side, width)
    d = _VAE_DEFAULT[side, width][1]
    if kind == "default":
        assert s["fold"] and s["mode"] == 1 and s["a2"] == s["a2_on_wf"] > 0 and s["shortcut_gemm"] == 0
        wit = f"conv3x3 with a2 {s['a2']}, shortcut GEMMs 0, stats1 {s['gn_stats']}"
    elif kind == "unfold":
        assert not s["fold"] and s["a2"] == 0 and s["shortcut_gemm"] == d["a2"] and s["gemm"] == d["gemm"] + d["a2"], (s, d)
        wit = f"conv3x3 with a2 {d['a2']} -> 0, GEMMs on conv_shortcut.w 0 -> {s['shortcut_gemm']}"
    else:
        mode = 0 if kind == "stats0" else 2
        assert s["mode"] == mode
        wit = witness_stats(s, d, mode, VAE_MORE_STATS[side, width])
    report(f"VAE {side} {width}: {env_name(env)}", "restatement case", err, wit)
    assert err < VAE_TOL


# ================================================================================================================ afterwards
def test_networks_are_left_with_default_engines(tiny, full):
    """No configuration above leaks: both module-scoped networks have no engine and no precision request, the library knob is
    unset, and the next engine is the default one (as a following tests/test_model_gpu.py needs it)."""
    from seva import ops
    assert _net_is_default(tiny[0]) and _net_is_default(full[0])
    assert ops.get_knob("attn_split") < 0
    from seva._engine import SPLIT_DEFAULT, parse_split
    eng = tiny[0].engine()
    try:
        assert not eng.fp8 and eng.ff_fused and eng.gn_fused_stats == 1 and eng.conv_splitk and eng.attn_split and not eng.fold_skip
        assert eng.attn_split_max == 2 and set(eng.split) == parse_split(SPLIT_DEFAULT)
    finally:
        tiny[0]._engine = None
