"""CPU checks of the e4m3 fused feed-forward option of the fp8 mode (`Seva.set_precision("fp8", ff="fp8")`): argument
validation, the engine's routing (a recorder of the new operator stands in for the kernel, fake_ops for the rest), the
restatement of the packed weight layouts (stable-virtual-camera_amd/csrc/ff_fp8.h) and the torch emulation of the kernel's
arithmetic that tests/test_ff_fp8_gpu.py compares the kernel against."""
import math
import os

import pytest
import torch

import fake_ops
from conftest import ROOT, rel_l2

STEP = 128


# ------------------------------------------------------------------ restatements
def feature_of(pos: torch.Tensor) -> torch.Tensor:
    """byte P = 64 q + 16 g + 8 c + r of a 128-feature step holds hidden feature 64 c + 32 q + 8 g + r"""
    q, g, c, r = pos >> 6, (pos >> 4) & 3, (pos >> 3) & 1, pos & 7
    return 64 * c + 32 * q + 8 * g + r


def e4m3(x: torch.Tensor) -> torch.Tensor:
    """saturating round-to-nearest-even to OCP e4m3, back to float32"""
    return x.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float()


def unpermute_w2(w2_8: torch.Tensor) -> torch.Tensor:
    """stored [C, 4C] -> natural column order"""
    n = w2_8.shape[1]
    i = torch.arange(n)
    perm = (i // STEP) * STEP + feature_of(i % STEP)
    out = torch.empty_like(w2_8)
    out[:, perm] = w2_8
    return out


def dequant(w8: torch.Tensor, w_exp: torch.Tensor) -> torch.Tensor:
    return w8.view(torch.float8_e4m3fn).double() * torch.exp2(w_exp.double() - 127.0)[:, None]


def layernorm_e4m3(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """The kernel's LayerNorm prologue: exact two-pass statistics in fp32, one e4m3 rounding of the normalised value."""
    x = x.float()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return e4m3((x - mean) * torch.rsqrt(var + eps) * gamma.float() + beta.float())


def ff_fp8_reference(a_q, w1_8, w1_exp, b1, w2_8, w2_exp, b2, residual=None) -> torch.Tensor:
    """The kernel's arithmetic in fp64: a_q [M, C] (e4m3 values), weights as `seva.ops.pack_ff_fp8` stores them.  GEGLU with
    the exact erf GELU, the hidden value rounded once to e4m3 (through fp32, as the kernel rounds its fp32 value)."""
    M, c = a_q.shape
    w1 = dequant(w1_8, w1_exp)[:, :c]
    h = (a_q.double() @ w1.T + b1.double()).view(M, 4 * c // 32, 2, 32)
    v, g = h[:, :, 0], h[:, :, 1]
    hid = e4m3((v * 0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0)))).reshape(M, 4 * c).float()).double()
    out = hid @ dequant(unpermute_w2(w2_8), w2_exp).T + b2.double()
    if residual is not None:
        out = out + residual.double()
    return out


def ff_fp32(x, gamma, beta, w1i, b1i, w2, b2, residual=None) -> torch.Tensor:
    """Unquantised feed-forward (interleaved W1) on LayerNorm(x), fp64."""
    a = torch.nn.functional.layer_norm(x.double(), (x.shape[-1],), gamma.double(), beta.double(), 1e-5)
    M, c = a.shape
    h = (a @ w1i.double().T + b1i.double()).view(M, 4 * c // 32, 2, 32)
    v, g = h[:, :, 0], h[:, :, 1]
    out = (v * torch.nn.functional.gelu(g)).reshape(M, 4 * c) @ w2.double().T + b2.double()
    return out if residual is None else out + residual.double()


def random_ff(c: int, g: torch.Generator):
    from seva._engine import interleave_geglu
    w1 = torch.randn(8 * c, c, generator=g) / math.sqrt(c)
    b1 = torch.randn(8 * c, generator=g) * 0.1
    w2 = torch.randn(c, 4 * c, generator=g) / math.sqrt(4 * c)
    b2 = torch.randn(c, generator=g) * 0.1
    w1i, b1i = interleave_geglu(w1, b1)
    return w1i.float().contiguous(), b1i.float().contiguous(), w2, b2


# ------------------------------------------------------------------ tests: layouts
def test_w2_order_is_a_bijection_matching_the_header():
    pos = torch.arange(STEP)
    f = feature_of(pos)
    assert torch.equal(torch.sort(f).values, pos)
    # lane group g, lo half (q = 0): chunk c = 0 then 1, 8 features each
    assert f[:16].tolist() == list(range(8)) + list(range(64, 72))
    assert f[64:72].tolist() == list(range(32, 40))  # hi half (q = 1), lane group 0
    # the header's formula, restated as written there
    src = open(os.path.join(ROOT, "stable-virtual-camera_amd", "csrc", "ff_fp8.h")).read()
    assert "64 * ((pos >> 3) & 1) + 32 * (pos >> 6) + 8 * ((pos >> 4) & 3) + (pos & 7)" in src
    from seva import ops
    assert torch.equal(ops.ff8_feature_of(pos), f)


@pytest.mark.parametrize("c", [64, 128, 256, 320])
def test_pack_pads_w1_and_permutes_w2(c):
    from seva import ops
    g = torch.Generator().manual_seed(c)
    w1i, _, w2, _ = random_ff(c, g)
    w1_8, w1_exp, w2_8, w2_exp = ops.pack_ff_fp8(w1i, w2)
    kp = (c + 127) // 128 * 128
    assert w1_8.shape == (8 * c, kp) and w1_8.dtype == torch.uint8 and w1_exp.shape == (8 * c,)
    assert w2_8.shape == (c, 4 * c) and w2_exp.shape == (c,) and w1_8.is_contiguous() and w2_8.is_contiguous()
    assert (w1_8[:, c:] == 0).all()  # e4m3 +0
    q1, e1 = ops.quantize_weight_fp8(w1i)
    assert torch.equal(w1_8[:, :c], q1) and torch.equal(w1_exp, e1)
    q2, e2 = ops.quantize_weight_fp8(w2)
    assert torch.equal(unpermute_w2(w2_8), q2) and torch.equal(w2_exp, e2)
    # whole-step bijection: every step's bytes come from that step's columns only
    assert torch.equal(torch.sort(w2_8.view(c, -1, STEP), -1).values, torch.sort(q2.view(c, -1, STEP), -1).values)


def test_emulation_against_the_unquantised_feed_forward():
    from seva import ops
    g = torch.Generator().manual_seed(3)
    for c in (64, 320):
        w1i, b1i, w2, b2 = random_ff(c, g)
        x = torch.randn(300, c, generator=g) * 2 + 0.5
        gamma, beta = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
        res = torch.randn(300, c, generator=g)
        w1_8, w1_exp, w2_8, w2_exp = ops.pack_ff_fp8(w1i, w2)
        out = ff_fp8_reference(layernorm_e4m3(x, gamma, beta), w1_8, w1_exp, b1i, w2_8, w2_exp, b2, res)
        ref = ff_fp32(x, gamma, beta, w1i, b1i, w2, b2, res)
        err = rel_l2(out - res.double(), ref - res.double())
        print(f"C={c}: e4m3 emulation vs fp32 feed-forward (residual excluded): rel-L2 {err:.3e}")
        assert 5e-3 < err < 8e-2, err  # the e4m3 class: three roundings to 3 mantissa bits


# ------------------------------------------------------------------ tests: API
def test_set_precision_validates_the_ff_option():
    from seva.model import Seva, SevaParams
    with torch.device("meta"):
        net = Seva(SevaParams(model_channels=64))
    assert net.set_precision("fp8", ff="fp8") is net and net._ff_precision == "fp8"
    net.set_precision("fp8", attention="fp8", ff="fp8")
    assert net._attention == "fp8" and net._ff_precision == "fp8"
    net.set_precision("fp8")
    assert net._ff_precision is None  # left to SEVA_FP8_FF
    net.set_precision("f16", ff="f16")
    with pytest.raises(ValueError, match="fp8"):
        net.set_precision("f16", ff="fp8")
    with pytest.raises(ValueError):
        net.set_precision("fp8", ff="int8")


# ------------------------------------------------------------------ tests: engine routing
def _fake_ops_with_ff8(calls):
    class Ops:
        pass

    from seva import ops as real
    ops = Ops()
    ops.__dict__.update({k: getattr(fake_ops, k) for k in dir(fake_ops) if not k.startswith("__")})
    ops.pack_ff_fp8 = real.pack_ff_fp8

    def ff_fused(*a, ln_x=None, **kw):
        calls.append(("ff16", ln_x.shape[-1]))
        return fake_ops.ff_fused(*a, ln_x=ln_x, **kw)

    def ff_fused_fp8(a, w1, w1_exp, b1, w2, w2_exp, b2, *, residual=None, out_f32=None, out_f16=None, ln_x=None,
                     ln_gamma=None, ln_beta=None, ln_eps=1e-5):
        assert a is None and ln_x is not None and ln_eps == 1e-5
        c = ln_x.shape[-1]
        x = ln_x.reshape(-1, c)
        M = x.shape[0]
        out = ff_fp8_reference(layernorm_e4m3(x, ln_gamma, ln_beta), w1, w1_exp, b1, w2, w2_exp, b2,
                               None if residual is None else residual.reshape(M, -1)[:, :c]).float()
        if out_f32 is not None:
            out_f32.view(M, -1)[:, :c].copy_(out)
        if out_f16 is not None:
            out_f16.view(M, -1)[:, :c].copy_(out.half())
        calls.append(("ff8", c))

    def gemm(a, w, **kw):
        calls.append(("gemm8" if kw.get("w_exp") is not None else "gemm16", a.shape[1], w.shape[0], bool(kw.get("geglu"))))
        return fake_ops.gemm(a, w, **kw)

    ops.ff_fused, ops.ff_fused_fp8, ops.gemm = ff_fused, ff_fused_fp8, gemm
    return ops


_ORIG_INIT = {}


def _engine_run(monkeypatch, precision, ff, env=None, extra_env=None):
    from seva import _engine
    from test_engine_host_logic import _cpu_engine
    calls = []
    monkeypatch.setattr(_engine, "ops", _fake_ops_with_ff8(calls))
    monkeypatch.setattr(_engine, "require_cuda", lambda *a: None)
    if env is not None:
        monkeypatch.setenv("SEVA_FP8_FF", env)
    else:
        monkeypatch.delenv("SEVA_FP8_FF", raising=False)
    for k, v in (extra_env or {}).items():
        monkeypatch.setenv(k, v)
    from seva._engine import SevaEngine
    orig = _ORIG_INIT.setdefault("init", SevaEngine.__init__)  # (a test may build two engines: never wrap the wrapper)
    monkeypatch.setattr(SevaEngine, "__init__", lambda self, m, p=None: orig(self, m, p, None, ff))
    eng, sd = _cpu_engine(precision=precision)
    T, h, w = 2, 16, 16
    g = torch.Generator().manual_seed(4)
    n = 2 * T
    x, t = torch.randn(n, 11, h, w, generator=g), torch.randint(0, 1000, (n,), generator=g)
    y, dense = torch.randn(n, 1, 1024, generator=g), torch.randn(n, 6, h, w, generator=g)
    out = eng.forward(x, None, t, y, dense, T)
    return eng, sd, calls, out, (x, t, y, dense, T)


def test_engine_routes_exactly_the_fused_feed_forwards(monkeypatch):
    from oracle import seva_ref as O
    _, _, base, _, _ = _engine_run(monkeypatch, "fp8", "f16")
    eng, sd, calls, out, args = _engine_run(monkeypatch, "fp8", "fp8")
    assert eng.ff8 and eng.ff == "fp8"
    ff16 = [c for kind, c, *_ in base if kind == "ff16"]
    assert ff16 and set(ff16) == {64}  # the tiny net: the C = 64 level takes the fused f16 kernel in fp8 mode
    # with the option: those calls, in the same order, go to the e4m3 kernel; every other call is unchanged
    assert [("ff8", c) if kind == "ff16" else (kind, c, *r) for kind, c, *r in base] == calls
    assert not any(kind == "ff16" for kind, *_ in calls)
    assert any(kind == "gemm8" for kind, *_ in calls)  # the C >= 128 feed-forwards stay on the two-kernel e4m3 chain
    err = rel_l2(out, O.seva_forward(sd, *args))
    print(f"fp8 mode + fp8 feed-forward (emulated kernels) vs fp32 oracle: rel-L2 {err:.3e}")
    assert 1e-3 < err < 0.15


@pytest.mark.parametrize("precision,ff,env", [("fp8", None, None), ("fp8", "f16", "1"), ("f16", None, None),
                                              ("f16", None, "1")])
def test_default_engines_never_take_the_fp8_feed_forward(monkeypatch, precision, ff, env):
    eng, _, calls, _, _ = _engine_run(monkeypatch, precision, ff, env)
    assert not eng.ff8 and not any(kind == "ff8" for kind, *_ in calls)
    assert any(kind == "ff16" for kind, *_ in calls)
    assert not any(k.endswith(".w1f8") for k in eng.W)  # the e4m3 copies are packed only with the option


def test_environment_switch_selects_the_fp8_feed_forward(monkeypatch):
    eng, _, calls, _, _ = _engine_run(monkeypatch, "fp8", None, "1")
    assert eng.ff8 and any(kind == "ff8" for kind, *_ in calls)


def test_option_changes_nothing_without_the_fused_feed_forward(monkeypatch):
    _, _, base, out0, _ = _engine_run(monkeypatch, "fp8", "f16", extra_env={"SEVA_FF_FUSED": "0"})
    _, _, calls, out1, _ = _engine_run(monkeypatch, "fp8", "fp8", extra_env={"SEVA_FF_FUSED": "0"})
    assert calls == base and torch.equal(out0, out1)


def test_engine_rejects_fp8_feed_forward_in_the_parity_mode(monkeypatch):
    with pytest.raises(ValueError, match="fp8"):
        _engine_run(monkeypatch, "f16", "fp8")
