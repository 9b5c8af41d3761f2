"""CPU checks of the fp8 P.V attention sub-option of the fp8 mode (`Seva.set_precision("fp8", attention="fp8")`): argument
validation, the engine's routing (fakes of the two new operators stand in for the kernels) and the torch restatements of the
quantised-V layout and of the kernel's arithmetic that tests/test_attention_fp8_gpu.py compares the kernels against."""
import math

import pytest
import torch

import fake_ops
from conftest import rel_l2

# ------------------------------------------------------------------ restatements (layout: stable-virtual-camera_amd/csrc/attn_pv8.h)
STEP = 128


def key_of(pos: torch.Tensor) -> torch.Tensor:
    """position p = 32 g + 4 kb + r of a 128-key step <-> key 16 kb + 4 g + r"""
    return 16 * ((pos >> 2) & 7) + 4 * (pos >> 5) + (pos & 3)


def group_pos() -> torch.Tensor:
    """[4, 32]: positions of scale group b -- 32 g + 16 (b >> 1) + jj for g in {2 (b & 1), 2 (b & 1) + 1}: the MFMA's reduction
    indices [32 b, 32 b + 32) (byte j of lane group g is k = 64 (j >> 4) + 16 g + (j & 15))"""
    b, j = torch.arange(4)[:, None], torch.arange(32)[None, :]
    return 32 * (2 * (b & 1) + (j >> 4)) + 16 * (b >> 1) + (j & 15)


def e8m0_exponent(amax: torch.Tensor) -> torch.Tensor:
    """quantize_weight_fp8's rule -- the smallest e with amax * 2^-e <= 448 -- evaluated exactly (frexp instead of a float log2,
    which can round at binade edges); all-zero groups take it at 1e-30; clamped to [-126, 127]"""
    m, E = torch.frexp(amax.float().clamp_min(1e-30))
    return torch.where(m <= 0.875, E - 9, E - 8).clamp(-126, 127)


def quantize_v_ref(v: torch.Tensor):
    """v: [B, L, H, 64] (f16 values) -> (values [B, H, S, 64, 128] uint8 as stored, scales [B, H, S, 256] uint8 as stored,
    dequantised V [B, H, L, 64] float64 -- what the kernel multiplies)."""
    B, L, H, D = v.shape
    S = (L + STEP - 1) // STEP
    vp = torch.zeros((B, S * STEP, H, D), dtype=torch.float32)
    vp[:, :L] = v.float()
    vs = vp.view(B, S, STEP, H, D)[:, :, key_of(torch.arange(STEP))]       # [B, S, pos, H, D]
    gpos = group_pos()                                                       # [b, 32] positions of scale group b
    grp = vs[:, :, gpos.reshape(-1)].view(B, S, 4, 32, H, D)
    e = e8m0_exponent(grp.abs().amax(3))                                     # [B, S, 4, H, D]
    q = (grp * torch.exp2(-e.float())[:, :, :, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    deq = q.float().double() * torch.exp2(e.double())[:, :, :, None]        # [B, S, 4, 32, H, D]
    # back to position order, then to key order
    deq_pos = torch.empty((B, S, STEP, H, D), dtype=torch.float64)
    deq_pos[:, :, gpos.reshape(-1)] = deq.reshape(B, S, STEP, H, D)
    qpos = torch.empty((B, S, STEP, H, D), dtype=torch.uint8)
    qpos[:, :, gpos.reshape(-1)] = q.view(torch.uint8).reshape(B, S, STEP, H, D)
    vhat = torch.empty_like(deq_pos)
    vhat[:, :, key_of(torch.arange(STEP))] = deq_pos
    vhat = vhat.reshape(B, S * STEP, H, D)[:, :L].permute(0, 2, 1, 3).contiguous()
    # stored value image: row = channel d, 16-byte chunk c at c ^ ((d >> 1) & 7)
    img = qpos.permute(0, 3, 1, 4, 2).contiguous()                           # [B, H, S, d, pos]
    d = torch.arange(D)
    chunk = torch.arange(8)
    phys = chunk[None, :] ^ ((d[:, None] >> 1) & 7)                          # [d, logical chunk] -> physical chunk
    stored = torch.empty_like(img).view(B, H, S, D, 8, 16)
    stored[:, :, :, d[:, None], phys] = img.view(B, H, S, D, 8, 16)[:, :, :, d[:, None], chunk[None, :]]
    # scales: byte 4 (16 b + (d & 15)) + (d >> 4)
    sc = torch.empty((B, H, S, 256), dtype=torch.uint8)
    eb = (e + 127).to(torch.uint8).permute(0, 3, 1, 2, 4)                    # [B, H, S, b, d]
    gg, dd = torch.meshgrid(torch.arange(4), d, indexing="ij")
    sc[:, :, :, (4 * (16 * gg + (dd & 15)) + (dd >> 4)).reshape(-1)] = eb.reshape(B, H, S, -1)
    return stored.view(B, H, S, D, STEP), sc, vhat


def pv8_reference(qs: torch.Tensor, k: torch.Tensor, vhat: torch.Tensor) -> torch.Tensor:
    """The kernel's arithmetic in fp64: q pre-scaled (log2 domain), s = q . k, P = e4m3(2^(s - M)) with the integer reference
    M = ceil(max s) - 8 (the kernel's reference is ceil(running maximum) - 8; e4m3 rounding commutes with integer powers of two, so
    only probabilities below e4m3's normal range relative to M could round differently), l = sum of the QUANTISED P,
    O = P vhat / l.  qs: [..., Lq, 64], k: [..., Lk, 64], vhat: [..., Lk, 64] (float64)."""
    s = qs.double() @ k.double().transpose(-1, -2)
    M = torch.ceil(s.amax(-1, keepdim=True)) - 8.0
    p = torch.exp2(s - M).float().to(torch.float8_e4m3fn).double()
    return (p @ vhat) / p.sum(-1, keepdim=True)


# ------------------------------------------------------------------ tests
def test_restatement_layout_is_a_permutation_of_whole_steps():
    pos = torch.arange(STEP)
    assert torch.equal(torch.sort(key_of(pos)).values, pos)
    # a lane group's 32 positions = 8 key blocks x 4 consecutive keys; a scale group = half of two lane groups' positions
    assert key_of(torch.arange(32)).tolist()[:8] == [0, 1, 2, 3, 16, 17, 18, 19]
    gp = group_pos()
    assert torch.equal(torch.sort(gp.reshape(-1)).values, pos) and gp[1, :4].tolist() == [64, 65, 66, 67]
    v = torch.randn(2, 300, 3, 64).half()
    stored, sc, vhat = quantize_v_ref(v)
    assert stored.shape == (2, 3, 3, 64, 128) and sc.shape == (2, 3, 3, 256)
    assert rel_l2(vhat.permute(0, 2, 1, 3).float(), v.float()) < 5e-2
    e = e8m0_exponent(torch.tensor([448.0, 449.0, 224.0, 224.5, 0.0, 1e-30, 65504.0]))
    assert e.tolist() == [0, 1, -1, 0, -108, -108, 8]


def test_restatement_of_the_arithmetic_against_fp64():
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(2, 500, 64, generator=g) for _ in range(3))
    qs = q * 0.125 * 1.4426950408889634
    _, _, vhat = quantize_v_ref(v.half().permute(1, 0, 2).unsqueeze(0))  # B = 1, H = 2 (the leading dim)
    out = pv8_reference(qs, k, vhat[0])
    ref = torch.softmax(qs.double() @ k.double().transpose(-1, -2) * math.log(2.0), -1) @ v.double()
    err = rel_l2(out, ref)
    assert 1e-3 < err < 1e-1, err


def test_set_precision_validates_the_attention_option():
    from seva.model import Seva, SevaParams
    with torch.device("meta"):
        net = Seva(SevaParams(model_channels=64))
    assert net.set_precision("fp8", attention="fp8") is net and net._attention == "fp8"
    net.set_precision("fp8")
    assert net._attention is None  # left to SEVA_FP8_ATTENTION
    net.set_precision("f16", attention="f16")
    with pytest.raises(ValueError, match="fp8"):
        net.set_precision("f16", attention="fp8")
    with pytest.raises(ValueError):
        net.set_precision("fp8", attention="int8")


# fakes of the new operators: the fake quantiser keeps the dequantised V by workspace, the fake kernel runs the restatement
_QUANT = {}


def _fake_ops_with_pv8(calls):
    class Ops:
        pass

    ops = Ops()
    ops.__dict__.update({k: getattr(fake_ops, k) for k in dir(fake_ops) if not k.startswith("__")})
    ops.PV8_MIN_LQ = 2048

    def v_fp8_workspace_numel(batch, heads, lk):
        s = batch * heads * ((lk + STEP - 1) // STEP)
        return s * (8192 + 256)

    def quantize_v_fp8(v, ws, *, nb0, nb1, heads, lk, k_strides):
        assert nb1 == 1 and ws.numel() >= v_fp8_workspace_numel(nb0, heads, lk)
        vv = torch.as_strided(v, (nb0, lk, heads, 64), (k_strides[0], k_strides[2], 64, 1), v.storage_offset())
        _QUANT[ws.data_ptr()] = quantize_v_ref(vv)[2]
        calls.append(("quant", lk))

    def attention_pv8(q, k, ws, out, *, nb0, nb1, heads, lq, lk, q_strides, k_strides, o_strides, split_ws=None):
        def view(t, st, L):
            return torch.as_strided(t, (nb0, L, heads, 64), (st[0], st[2], 64, 1), t.storage_offset()).permute(0, 2, 1, 3)
        o = pv8_reference(view(q, q_strides, lq), view(k, k_strides, lk), _QUANT[ws.data_ptr()])
        view(out, o_strides, lq).copy_(o.half())
        calls.append(("pv8", lq))

    def attention(*a, lq, **kw):
        calls.append(("f16", lq))
        return fake_ops.attention(*a, lq=lq, **kw)

    ops.v_fp8_workspace_numel, ops.quantize_v_fp8, ops.attention_pv8, ops.attention = (
        v_fp8_workspace_numel, quantize_v_fp8, attention_pv8, attention)
    return ops


def _engine_run(monkeypatch, precision, attention, env=None):
    from seva import _engine
    from test_engine_host_logic import _cpu_engine
    calls = []
    monkeypatch.setattr(_engine, "ops", _fake_ops_with_pv8(calls))
    monkeypatch.setattr(_engine, "require_cuda", lambda *a: None)
    if env is not None:
        monkeypatch.setenv("SEVA_FP8_ATTENTION", env)
    else:
        monkeypatch.delenv("SEVA_FP8_ATTENTION", raising=False)
    from seva._engine import SevaEngine
    orig = SevaEngine.__init__
    monkeypatch.setattr(SevaEngine, "__init__", lambda self, m, p=None: orig(self, m, p, attention))
    eng, sd = _cpu_engine(precision=precision)
    # T = 2 frames of 48 x 48 latents: per-frame attention at the top level has L = 2304 (>= 2048: pv8); the lower levels,
    # temporal (L = 2) and cross attention stay f16
    T, h, w = 2, 48, 48
    g = torch.Generator().manual_seed(4)
    n = 2 * T
    x, t = torch.randn(n, 11, h, w, generator=g), torch.randint(0, 1000, (n,), generator=g)
    y, dense = torch.randn(n, 1, 1024, generator=g), torch.randn(n, 6, h, w, generator=g)
    out = eng.forward(x, None, t, y, dense, T)
    return eng, sd, calls, out, (x, t, y, dense, T)


def test_engine_routes_exactly_the_long_self_attention_launches(monkeypatch):
    from oracle import seva_ref as O
    eng, sd, calls, out, args = _engine_run(monkeypatch, "fp8", "fp8")
    assert eng.pv8 and eng.attention == "fp8"
    pv8 = [lq for kind, lq in calls if kind == "pv8"]
    f16 = [lq for kind, lq in calls if kind == "f16"]
    assert 2304 in pv8 and all(lq >= 2048 for lq in pv8)
    assert f16 and all(lq < 2048 for lq in f16)
    assert [lq for kind, lq in calls if kind == "quant"] == pv8  # one V quantisation per pv8 launch, in front of it
    err = rel_l2(out, O.seva_forward(sd, *args))
    print(f"fp8 mode + fp8 attention (emulated kernels) vs fp32 oracle: rel-L2 {err:.3e}")
    assert 1e-3 < err < 0.15


@pytest.mark.parametrize("precision,attention,env", [("fp8", None, None), ("fp8", "f16", "1"), ("f16", None, None),
                                                     ("f16", None, "1")])
def test_default_engines_never_take_the_fp8_attention(monkeypatch, precision, attention, env):
    eng, _, calls, _, _ = _engine_run(monkeypatch, precision, attention, env)
    assert not eng.pv8 and not any(kind in ("pv8", "quant") for kind, _ in calls)
    assert any(lq >= 2048 for kind, lq in calls if kind == "f16")


def test_environment_switch_selects_the_fp8_attention(monkeypatch):
    eng, _, calls, _, _ = _engine_run(monkeypatch, "fp8", None, "1")
    assert eng.pv8 and any(kind == "pv8" for kind, _ in calls)


def test_engine_rejects_fp8_attention_in_the_parity_mode(monkeypatch):
    with pytest.raises(ValueError, match="fp8"):
        _engine_run(monkeypatch, "f16", "fp8")
