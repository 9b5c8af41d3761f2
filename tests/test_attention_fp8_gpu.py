"""fp8 P.V attention (seva_attn_quant_v_fp8 + seva_attention_pv8), the opt-in attention sub-option of the fp8 mode: the V
quantiser bit for bit against its torch restatement, the kernel against fp64 fed the same quantised V and the same P rounding,
against unquantised fp64 (loosely), around its rescale bound, batch invariance, the 1.3B network at the headline shape, and the
whole-step hipGraph.  Restatements: tests/test_attention_fp8_cpu.py."""
import math

import pytest
import torch

from conftest import rel_l2
from test_attention_fp8_cpu import pv8_reference, quantize_v_ref

pytestmark = pytest.mark.gpu
QK_C = 0.125 * 1.4426950408889634


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from seva import _native
    _native.load()
    return torch.device("cuda:0")


def _qkv(B, H, Lq, Lk, seed, spread=1.0):
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn((B, Lq, H, 64), generator=g) * spread * QK_C).half()
    k = torch.randn((B, Lk, H, 64), generator=g).half()
    v = torch.randn((B, Lk, H, 64), generator=g).half()
    return q, k, v


def _run(dev, q, k, v, split=False, out_nan=True):
    """packed [B, L, 3C]-style strides are not needed here: q / k / v are separate [B, L, H * 64] tensors"""
    from seva import ops
    B, Lq, H, _ = q.shape
    Lk = k.shape[1]
    C = 64 * H
    q16, k16, v16 = q.to(dev).reshape(B, Lq, C), k.to(dev).reshape(B, Lk, C), v.to(dev).reshape(B, Lk, C)
    ws = torch.empty(ops.v_fp8_workspace_numel(B, H, Lk), dtype=torch.uint8, device=dev)
    out = torch.full((B, Lq, C), float("nan") if out_nan else 0.0, device=dev, dtype=torch.float16)
    sws = torch.empty(ops.attention_split_workspace_numel(B, H, Lq), dtype=torch.float32, device=dev) if split else None
    ops.quantize_v_fp8(v16, ws, nb0=B, nb1=1, heads=H, lk=Lk, k_strides=(Lk * C, 0, C))
    ops.attention_pv8(q16, k16, ws, out, nb0=B, nb1=1, heads=H, lq=Lq, lk=Lk, q_strides=(Lq * C, 0, C),
                      k_strides=(Lk * C, 0, C), o_strides=(Lq * C, 0, C), split_ws=sws)
    torch.cuda.synchronize()
    return out.view(B, Lq, H, 64), ws


def _rows(Lq, n=192, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = torch.randperm(Lq, generator=g)[:n]
    return torch.unique(torch.cat([r, torch.arange(max(0, Lq - 40), Lq), torch.arange(min(40, Lq))]))


def _ref(dev, q, k, vhat, rows):
    """pv8_reference of the sampled query rows, on the GPU in fp64: [B, len(rows), H, 64]"""
    qs = q[:, rows].permute(0, 2, 1, 3).to(dev)
    o = pv8_reference(qs, k.permute(0, 2, 1, 3).to(dev), vhat.to(dev))
    return o.permute(0, 2, 1, 3).cpu()


def _exact(dev, q, k, v, rows):
    qd = q[:, rows].permute(0, 2, 1, 3).double().to(dev)
    kd, vd = k.permute(0, 2, 1, 3).double().to(dev), v.permute(0, 2, 1, 3).double().to(dev)
    return (torch.softmax(qd @ kd.transpose(-1, -2) * math.log(2.0), -1) @ vd).permute(0, 2, 1, 3).cpu()


@pytest.mark.parametrize("B,H,L", [(2, 3, 1000), (1, 2, 27216), (3, 1, 129)])
def test_v_quantiser_is_bit_exact(dev, B, H, L):
    q, k, v = _qkv(B, H, 8, L, seed=L)
    v[0, :40, 0] = 0.0                      # an all-zero scale group
    v[0, 40 % L, 0, :8] = 448.0             # values at +-448 (a group whose maximum is exactly the e4m3 maximum)
    v[0, 41 % L, 0, 8:16] = -448.0
    v[-1, -3:, -1] *= 1000.0                # large values in the last, zero-padded step
    _, ws = _run(dev, q[:, :8], k, v)
    stored, sc, _ = quantize_v_ref(v)
    S = stored.shape[2]
    n8 = B * H * S * 8192
    got_v = ws[:n8].cpu().view(B, H, S, 64, 128)
    got_s = ws[n8:n8 + B * H * S * 256].cpu().view(B, H, S, 256)
    assert torch.equal(got_s, sc)
    assert torch.equal(got_v, stored)


def test_v_quantiser_scale_groups_do_not_straddle_scenes(dev):
    """27216 = 212.6 steps of 128: the last step of scene 0 is zero-padded, scene 1 starts a fresh step; a huge value in the first
    key of scene 1 must not change any scale byte of scene 0"""
    B, H, L = 2, 1, 27216
    q, k, v = _qkv(B, H, 8, L, seed=3)
    _, ws0 = _run(dev, q, k, v)
    v2 = v.clone()
    v2[1, 0] = 30000.0
    _, ws1 = _run(dev, q, k, v2)
    S = (L + 127) // 128
    n8 = B * H * S * 8192
    sc0, sc1 = ws0[n8:].cpu().view(B, S, 256), ws1[n8:].cpu().view(B, S, 256)
    assert torch.equal(sc0[0], sc1[0]) and not torch.equal(sc0[1, 0], sc1[1, 0])


SHAPES = [(2, 10, 27216, 27216, True), (2, 10, 27216, 27216, False), (42, 5, 5184, 5184, False), (2, 20, 6804, 6804, True),
          (3, 2, 2311, 2311, False), (2, 3, 2048, 1000, False), (1, 4, 3000, 7001, True), (2, 2, 4100, 77, False)]


@pytest.mark.parametrize("B,H,Lq,Lk,split", SHAPES)
def test_kernel_does_the_stated_arithmetic(dev, B, H, Lq, Lk, split):
    q, k, v = _qkv(B, H, Lq, Lk, seed=Lq + Lk, spread=2.0)
    out, _ = _run(dev, q, k, v, split=split)
    assert torch.isfinite(out).all()
    rows = _rows(Lq)
    _, _, vhat = quantize_v_ref(v)
    got = out[:, rows].cpu().double()
    err = rel_l2(got, _ref(dev, q, k, vhat, rows))
    err_q = rel_l2(got, _exact(dev, q, k, v, rows))
    print(f"\npv8 B={B} H={H} Lq={Lq} Lk={Lk} split={split}: vs its own arithmetic in fp64 {err:.2e}; vs unquantised fp64 {err_q:.2e}")
    assert err < 4e-3
    assert 1e-3 < err_q < 1e-1


@pytest.mark.parametrize("above", [4.0, 7.9, 8.0, 8.5, 12.0, 20.0])
def test_kernel_late_key_around_the_rescale_bound(dev, above):
    """pv8_kernel rescales when a score passes its integer running reference by 8 (P <= 256 < 448): a late key whose score lies
    `above` log2 units over the first part's maximum walks below, at and above that bound, in the first and the later parts of a
    tile.  Outputs stay finite and agree with the kernel's arithmetic in fp64."""
    B, H, Lq, Lk = 1, 2, 2304, 700
    g = torch.Generator().manual_seed(5)
    q = torch.randn((B, Lq, H, 64), generator=g)
    k = torch.randn((B, Lk, H, 64), generator=g)
    v = torch.randn((B, Lk, H, 64), generator=g).half()
    qs = (q * QK_C).half()
    s0 = torch.einsum("blhd,bkhd->bhlk", qs.double(), k[:, :32].half().double()).amax(-1)
    for h in range(H):
        d = qs[0, 0, h].double()
        for key in (200, 300, 470):  # second / third part of tile 1, last part of tile 3
            k[0, key, h] = (d / d.dot(d) * (float(s0[0, h, 0]) + above)).float()
    k = k.half()
    out, _ = _run(dev, qs, k, v)
    assert torch.isfinite(out).all()
    rows = _rows(Lq)
    _, _, vhat = quantize_v_ref(v)
    got = out[:, rows].cpu().double()
    err = rel_l2(got, _ref(dev, qs, k, vhat, rows))
    err0 = rel_l2(out[:, :1].cpu().double(), _ref(dev, qs, k, vhat, torch.tensor([0])))
    print(f"\nlate key {above:4.1f} above: vs the kernel's arithmetic in fp64 {err:.2e}, the targeted row {err0:.2e}")
    assert err < 4e-3 and err0 < 4e-3


def test_batch_invariance_and_determinism(dev):
    B, H, L = 2, 4, 6804
    q, k, v = _qkv(B, H, L, L, seed=11)
    both, _ = _run(dev, q, k, v, split=True)
    again, _ = _run(dev, q, k, v, split=True)
    alone, _ = _run(dev, q[1:], k[1:], v[1:], split=True)
    assert torch.equal(both, again)
    assert torch.equal(both[1:], alone)


def test_fp8_attention_forward_at_the_headline_shape_vs_reference(dev):
    """fp8 mode + attention="fp8", ONE 1.3B network call at T=21, 576x576 (B=42) against the reference's own output, beside the
    plain fp8 mode.  Bounded like the fp8 mode (< 6e-2 overall, < 1e-1 per latent) and must differ from the plain fp8 output."""
    import os
    from conftest import GOLD, load_golden
    from test_headline_gpu import FORWARD_SEEDS, _wrapper_inputs
    from test_model_gpu import _build
    from seva.model import SGMWrapper
    if not os.path.exists(os.path.join(GOLD, "g9_T21_forward.npz")):
        pytest.skip("g9_T21_forward.npz not generated")
    g = load_golden("g9_T21_forward")
    T = 21
    net, _ = _build("full", dev)
    x, t, c = _wrapper_inputs(T, FORWARD_SEEDS[T])
    run = lambda: SGMWrapper(net)(x.to(dev), t.to(dev), {k: v.to(dev) for k, v in c.items()}, num_frames=T).cpu()  # noqa: E731
    net.set_precision("fp8", attention="f16")
    y8 = run()
    net.set_precision("fp8", attention="fp8")
    y = run()
    assert net.engine().pv8
    ref = g["y"]
    err, err8 = rel_l2(y, ref), rel_l2(y8, ref)
    per = [rel_l2(y[i], ref[i]) for i in range(y.shape[0])]
    print(f"\nfp8 mode + fp8 attention, 1.3B forward T=21 72x72 (B=42) vs REFERENCE: rel-L2 {err:.3e}; per latent max {max(per):.3e} "
          f"(plain fp8 mode: {err8:.3e})")
    assert torch.isfinite(y).all() and not torch.equal(y, y8)
    assert err < 6e-2 and max(per) < 1e-1


def test_whole_step_graph_equals_eager_in_the_fp8_attention_mode(dev, monkeypatch):
    """tiny network at 48 x 48 latents (per-frame L = 2304, joint 9216 with the K/V split: both on pv8_kernel), 4-step loop: whole-step
    hipGraph replay against the all-eager loop, bit for bit"""
    from test_model_gpu import _build, _loop
    net, _ = _build("tiny", dev)
    net.set_precision("fp8", attention="fp8")
    T, hw, steps = 4, 48, 4
    g = torch.Generator().manual_seed(5)
    eps = [torch.randn(T, 4, hw, hw, generator=g) for _ in range(steps)]
    monkeypatch.setenv("SEVA_STEPGRAPH", "0")
    monkeypatch.setenv("SEVA_HIPGRAPH", "0")
    ref, s0 = _loop(net, dev, T, hw, steps, eps)
    assert net.engine().pv8 and s0._step_graphs.captures == 0
    monkeypatch.setenv("SEVA_STEPGRAPH", "1")
    monkeypatch.setenv("SEVA_HIPGRAPH", "1")
    got, s1 = _loop(net, dev, T, hw, steps, eps)
    assert s1._step_graphs.captures == 1
    assert torch.isfinite(got).all() and torch.equal(got, ref)
