"""Engine switches on the CPU emulation (tests/fake_ops.py), and the machinery tests/test_engine_switches_gpu.py shares with it.

`SevaEngine.__init__` reads about a dozen environment switches; each selects other kernels, operand layouts or weight packings.
Every test here builds an engine under ONE configuration, runs one eager forward with a call recorder wrapped around the operator
module, and asserts two things: the result stays inside the bound of its class, and the recorded calls prove that the switch changed
what ran (a silently ignored switch would pass the first check alone).  Witnesses are relations between recordings ("no call to
ff_fused", "some conv3x3 got a2 and fewer gemm calls than the default"), never call counts.

The forward is the eager launch sequence (`engine.forward`): one pass, one recording.  (The hipGraph replay is pinned bit-equal to
it in tests/test_model_gpu.py.)

This file keeps the folded-weight packing (`conv2.wf` / `conv2.bf`) and the statistics hand-off honest without a GPU: bound
`err < 2e-3` against the reference golden / the fp32 oracle, the bound of tests/test_engine_host_logic.py for emulated kernels.
"""
import contextlib

import pytest
import torch

import fake_ops
from conftest import load_golden, rel_l2

# every switch an engine constructor (or `_resample`) reads: a configuration starts from a state with all of them removed
ENGINE_SWITCHES = (
    "SEVA_PRECISION", "SEVA_FP8_ATTENTION", "SEVA_FP8_FF", "SEVA_FP8_PAD", "SEVA_FF_FUSED", "SEVA_GN_FUSED_STATS",
    "SEVA_CONV_SPLITK", "SEVA_ATTN_SPLIT_KV", "SEVA_ATTN_SPLIT", "SEVA_FOLD_SKIP", "SEVA_SPLIT_PRECISION", "SEVA_UPSAMPLE_PHASES",
    "SEVA_SLICE_FRAMES", "SEVA_SLICE_MIN_MB", "SEVA_SLICE_ATTN", "SEVA_VAE_FOLD_SHORTCUT", "SEVA_VAE_PRECISION",
    "SEVA_VAE_ENCODE_PRECISION", "SEVA_VAE_UPSAMPLE_PHASES", "SEVA_VAE_FP8_DOWNSAMPLE", "SEVA_VAE_FP8_UPSAMPLE")

# the operators whose calls tell the configurations apart (wrapped where the module has them)
RECORDED_OPS = (
    "gemm", "gemm_split_out", "conv3x3", "conv3x3_up_phases", "conv3x3_up_phases128", "ff_fused", "ff_fused_fp8", "attention",
    "attention_pv8", "quantize_v_fp8", "groupnorm", "layernorm", "layernorm_split", "cast_concat_f16_split", "nchw_to_nhwc_f16")


class TensorArg:
    """What the recorder keeps of a tensor argument (never the tensor: a recording must not keep an engine's buffers alive)."""
    __slots__ = ("shape", "dtype", "ptr")

    def __init__(self, t):
        self.shape, self.dtype, self.ptr = tuple(t.shape), t.dtype, t.data_ptr()


def _describe(v):
    if isinstance(v, torch.Tensor):
        return TensorArg(v)
    if isinstance(v, (tuple, list)):
        return tuple(_describe(e) for e in v)
    return v


class Call:
    __slots__ = ("name", "args", "kw")

    def __init__(self, name, args, kw):
        self.name, self.args, self.kw = name, args, kw

    def given(self, key) -> bool:
        """Was keyword `key` passed with something that switches a feature on (a tensor, True, a non-zero number)?"""
        v = self.kw.get(key)
        if isinstance(v, TensorArg):
            return True
        return v is not None and v is not False and v != 0


class Recorder:
    """Wraps the functions of an operator module: every call is recorded (shapes, dtypes, pointers, plain keyword values), then made."""

    def __init__(self, mp, module):
        self.calls: list = []
        for name in RECORDED_OPS:
            real = getattr(module, name, None)
            if real is not None:
                mp.setattr(module, name, self._wrap(name, real))

    def _wrap(self, name, real):
        def recorded(*a, **k):
            self.calls.append(Call(name, tuple(_describe(v) for v in a), {key: _describe(v) for key, v in k.items()}))
            return real(*a, **k)

        return recorded

    def named(self, *names) -> list:
        return [c for c in self.calls if c.name in names]

    def count(self, name, pred=None) -> int:
        return sum(1 for c in self.calls if c.name == name and (pred is None or pred(c)))


@contextlib.contextmanager
def switched(monkeypatch, ops_module, env, build, drop=None):
    """One configuration: the environment holds exactly `env` of the engine switches, `build()` constructs the engine under it (the
    switches are read at construction), the body runs with a recorder around `ops_module`; afterwards the environment and the
    operator module are as before and `drop()` has taken the engine away again, also when the body raised."""
    with monkeypatch.context() as mp:
        for k in ENGINE_SWITCHES:
            mp.delenv(k, raising=False)
        for k, v in env.items():
            assert k in ENGINE_SWITCHES, k
            mp.setenv(k, str(v))
        rec = Recorder(mp, ops_module)
        try:
            yield build(), rec
        finally:
            if drop is not None:
                drop()


def env_name(env) -> str:
    return "default" if not env else " ".join(f"{k[5:]}={v}" for k, v in env.items())


def report(config, inp, err, witness) -> None:
    """One line of the table in profiles/engine_switches.log."""
    print(f"\n[switch] {config:44s} | {inp:22s} | rel-L2 {err:.3e} | {witness}")


# ------------------------------------------------------------------------------------------------------------------ inputs
def golden_inputs(name):
    g = load_golden(name)
    return (g["x"], g["concat"], g["t"], g["crossattn"], g["dense_vector"], int(g["T"])), g["y"]


def random_inputs(T, h, w, n=None):
    """The inputs of tests/test_model_gpu.py::test_tiny_forward_odd_shapes (same seeds), n = 2 T unless given."""
    g = torch.Generator().manual_seed(T * 100 + h)
    n = n or 2 * T
    x, t = torch.randn(n, 11, h, w, generator=g), torch.randint(0, 1000, (n,), generator=g)
    y, dense = torch.randn(n, 1, 1024, generator=g), torch.randn(n, 6, h, w, generator=g)
    return (x, None, t, y, dense, T)


_ORACLE: dict = {}


def oracle_reference(sd, key, inputs) -> torch.Tensor:
    """fp32 CPU oracle of the tiny network on `inputs`, computed once per shape and shared (never modified)."""
    if key not in _ORACLE:
        from oracle import seva_ref as O
        torch.set_num_threads(min(16, torch.get_num_threads()))
        x, concat, t, y, dense, T = inputs
        assert concat is None
        _ORACLE[key] = O.seva_forward(sd, x, t, y, dense, T)
    return _ORACLE[key]


# ------------------------------------------------------------------------------------------------------------------ witnesses
def summary(rec) -> dict:
    """The figures the witnesses compare between a configuration and the default of the same input."""
    gn = rec.named("groupnorm")
    convs = rec.named("conv3x3")
    return {
        "gemm": rec.count("gemm"),
        "ff_fused": rec.count("ff_fused"),
        "a2": sum(c.given("a2") for c in convs),
        "splitk_ws": sum(c.given("splitk_ws") for c in convs + rec.named("gemm")),
        "gn_stats": sum(c.given("stats1") for c in gn),
        "gn_stats2": sum(c.given("stats2") for c in gn),
        "ch_stats": sum(c.given("ch_stats") for c in convs + rec.named("gemm")),
        "changing": sum(c.given("raw_f16") for c in gn),  # channel-changing ResBlocks: their first GroupNorm emits the raw input
    }


def witness_ff_unfused(s, d):
    assert d["ff_fused"] > 0 and s["ff_fused"] == 0 and s["gemm"] > d["gemm"], (s, d)
    return f"ff_fused {d['ff_fused']} -> 0, gemm {d['gemm']} -> {s['gemm']}"


def witness_stats(s, d, mode, more):
    """SEVA_GN_FUSED_STATS=0: nothing emits or reads statistics.  =2: never fewer hand-offs than the default, and strictly more
    where the input has a level that only mode 2 takes (`more`: hw % 64 == 0 and c >= 128 with fewer than 16 tiles per sample)."""
    if mode == 0:
        assert s["gn_stats"] == 0 and s["gn_stats2"] == 0 and s["ch_stats"] == 0, s
    else:
        assert s["gn_stats"] >= d["gn_stats"] and s["ch_stats"] >= s["gn_stats"], (s, d)
        if more:
            assert s["gn_stats"] > d["gn_stats"] and s["ch_stats"] > d["ch_stats"], (s, d)
        else:
            assert s["gn_stats"] == d["gn_stats"], (s, d)
    return f"groupnorm with stats1 {d['gn_stats']} -> {s['gn_stats']}, producers with ch_stats {d['ch_stats']} -> {s['ch_stats']}"


def witness_no_splitk(s, d):
    assert d["splitk_ws"] > 0 and s["splitk_ws"] == 0, (s, d)
    return f"splitk_ws {d['splitk_ws']} -> 0"


def witness_fold(s, d, everywhere, some):
    """SEVA_FOLD_SKIP=1.  `everywhere` (with SEVA_CONV_SPLITK=0): every channel-changing ResBlock folds.  Otherwise only the levels
    of more than 128 pixels do: `some` says whether the input has such a level with a channel-changing ResBlock."""
    assert d["a2"] == 0 and d["changing"] > 0 and s["changing"] == d["changing"], (s, d)
    if everywhere:
        assert s["a2"] == s["changing"], s
    elif some:
        assert 0 < s["a2"] <= s["changing"], s
    else:
        assert s["a2"] == 0, s
    assert s["gemm"] == d["gemm"] - s["a2"], (s, d)  # each fold takes exactly the skip GEMM away
    return f"conv3x3 with a2 {s['a2']} of {s['changing']} channel-changing ResBlocks, gemm {d['gemm']} -> {s['gemm']}"


def check_folded_operands(rec, eng):
    """Every folded conv reads the raw-input buffer its ResBlock's first GroupNorm wrote, against a `conv2.wf` of the engine."""
    raw = {c.kw["raw_f16"].ptr: c for c in rec.named("groupnorm") if c.given("raw_f16")}
    wf = {v.data_ptr(): k for k, v in eng.W.items() if k.endswith(".conv2.wf")}
    bf = {v.data_ptr() for k, v in eng.W.items() if k.endswith(".conv2.bf")}
    folds = []
    for c in rec.named("conv3x3"):
        if c.given("a2"):
            a2, x, w = c.kw["a2"], c.args[0], c.args[1]
            assert a2.ptr in raw and w.ptr in wf and c.kw["bias"].ptr in bf and not c.given("residual")
            assert w.shape[1] == 9 * x.shape[-1] + a2.shape[1]
            cin, split = sum(t.shape[-1] for t in raw[a2.ptr].args[:2] if t is not None), raw[a2.ptr].given("split_raw")
            assert a2.shape[1] == (2 if split else 1) * cin
            folds.append({"cout": w.shape[0], "cin": cin, "k2": a2.shape[1], "split": split})
    return folds


# ------------------------------------------------------------------------------------------------------------------ CPU tests
TOL_EMULATED = 2e-3  # tests/test_engine_host_logic.py: emulated kernels against the golden / the oracle

# (environment, witness kind)
CPU_CONFIGS = [
    ({"SEVA_FOLD_SKIP": 1}, "fold"),
    ({"SEVA_FOLD_SKIP": 1, "SEVA_CONV_SPLITK": 0}, "fold_all"),
    ({"SEVA_FF_FUSED": 0}, "ff"),
    ({"SEVA_CONV_SPLITK": 0}, "splitk"),
    ({"SEVA_GN_FUSED_STATS": 0}, "stats0"),
    ({"SEVA_GN_FUSED_STATS": 2}, "stats2"),
]
# input -> (has a level of more than 128 pixels with a channel-changing ResBlock, has a level only SEVA_GN_FUSED_STATS=2 takes)
#   g3 (16x16): 256 pixels at the top, where the decoder's 128 -> 64 ResBlocks sit; 64 pixels x 128 channels one level down.
#   (3, 8, 24): 192 pixels at the top; below it 48 and 12 pixels, no multiple of 64.
CPU_INPUTS = {"g3": (True, True), "T3_8x24": (True, False)}


def _cpu_inputs(key):
    if key == "g3":
        return golden_inputs("g3_tiny_forward")
    return random_inputs(3, 8, 24), None


@pytest.fixture()
def emulated(monkeypatch):
    from seva import _engine
    monkeypatch.setattr(_engine, "ops", fake_ops)
    monkeypatch.setattr(_engine, "require_cuda", lambda *a: None)


_CPU_DEFAULT: dict = {}


def _cpu_run(monkeypatch, env, key):
    from test_engine_host_logic import _cpu_engine
    inputs, ref = _cpu_inputs(key)
    sd_box = []

    def build():
        eng, sd = _cpu_engine()
        sd_box.append(sd)
        return eng

    with switched(monkeypatch, fake_ops, env, build) as (eng, rec):
        out = eng.forward(*inputs).clone()
        check_folded_operands(rec, eng)
        facts = {"fold_skip": eng.fold_skip, "gn_fused_stats": eng.gn_fused_stats, "conv_splitk": eng.conv_splitk,
                 "ff_fused": eng.ff_fused}
    if ref is None:
        ref = oracle_reference(sd_box[0], key, inputs)
    return rel_l2(out, ref), summary(rec), facts


def _cpu_default(monkeypatch, key):
    if key not in _CPU_DEFAULT:
        _CPU_DEFAULT[key] = _cpu_run(monkeypatch, {}, key)
    return _CPU_DEFAULT[key]


@pytest.mark.parametrize("key", list(CPU_INPUTS))
def test_default_engine_emulated(emulated, monkeypatch, key):
    err, s, facts = _cpu_default(monkeypatch, key)
    report("default", key, err, f"ff_fused {s['ff_fused']}, gemm {s['gemm']}, splitk_ws {s['splitk_ws']}, stats {s['gn_stats']}")
    assert facts == {"fold_skip": False, "gn_fused_stats": 1, "conv_splitk": True, "ff_fused": True}
    assert s["ff_fused"] > 0 and s["splitk_ws"] > 0 and s["a2"] == 0
    assert err < TOL_EMULATED


@pytest.mark.parametrize("key", list(CPU_INPUTS))
@pytest.mark.parametrize("env,kind", CPU_CONFIGS, ids=[env_name(e) for e, _ in CPU_CONFIGS])
def test_switch_emulated(emulated, monkeypatch, env, kind, key):
    _, d, _ = _cpu_default(monkeypatch, key)
    err, s, facts = _cpu_run(monkeypatch, env, key)
    some_fold, more_stats = CPU_INPUTS[key]
    if kind == "fold":
        wit = witness_fold(s, d, False, some_fold)
    elif kind == "fold_all":
        wit = witness_fold(s, d, True, some_fold) + "; " + witness_no_splitk(s, d)
    elif kind == "ff":
        wit = witness_ff_unfused(s, d)
    elif kind == "splitk":
        wit = witness_no_splitk(s, d)
    else:
        mode = 0 if kind == "stats0" else 2
        assert facts["gn_fused_stats"] == mode
        wit = witness_stats(s, d, mode, more_stats)
    report(env_name(env), key, err, wit)
    assert err < TOL_EMULATED


def test_switches_leave_no_trace(emulated, monkeypatch):
    """After a configuration the environment and the operator module are as they were."""
    import os
    before = {k: os.environ.get(k) for k in ENGINE_SWITCHES}
    real = fake_ops.gemm
    with pytest.raises(RuntimeError, match="inside"):
        with switched(monkeypatch, fake_ops, {"SEVA_FOLD_SKIP": 1, "SEVA_CONV_SPLITK": 0}, lambda: None):
            assert os.environ["SEVA_FOLD_SKIP"] == "1" and fake_ops.gemm is not real
            raise RuntimeError("inside")
    assert {k: os.environ.get(k) for k in ENGINE_SWITCHES} == before and fake_ops.gemm is real
