"""Split-precision operands on the GPU: the three producers (seva_layernorm_f16_split, seva_cast_concat_f16_split,
seva_gemm_f16_split_out), a split operand through the consumers, and the network under `Seva.set_precision("f16", split="all")`
against the prediction of tests/test_split_operands_cpu.py.

Bounds.  LayerNorm: hi is the plain kernel's output bit for bit; hi + lo is the kernel's fp32 value carried to ~22 bits, checked
against an fp64 LayerNorm with the rel-L2 error seva_layernorm_f32 shows on the same inputs, times 2 (the lo half adds about
0.15 * 2^-22 relative rms to a value whose own fp32 evaluation error is of the same size or above: the sum in quadrature stays
below twice the latter).  GEMM / conv checks are on integer data and exact.  Network: 1.5 x the CPU prediction for the shape (fp32
accumulation order is all the prediction lacks).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from conftest import load_golden, rel_l2
from test_split_operands_cpu import PRED_CONFIG1, PRED_TINY

F16, F32 = torch.float16, torch.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from seva import _native
    _native.load()
    return torch.device("cuda:0")


def _hilo(v):
    hi = v.half()
    return hi, (v - hi.float()).half()


def _bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------------------ producers
@pytest.mark.parametrize("c", [64, 320, 1280])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1000])
def test_layernorm_split(dev, rows, c):
    from seva import ops
    g = torch.Generator().manual_seed(rows * 7 + c)
    x = (torch.randn(rows, c, generator=g) * 2 + 0.5).to(dev)
    gamma, beta = (1 + 0.3 * torch.randn(c, generator=g)).to(dev), (0.2 * torch.randn(c, generator=g)).to(dev)
    plain = torch.empty((rows, c), dtype=F16, device=dev)
    split = torch.full((rows, 2 * c), float("nan"), dtype=F16, device=dev)
    y32 = torch.empty((rows, c), dtype=F32, device=dev)
    ops.layernorm(x, gamma, beta, plain)
    ops.layernorm_split(x, gamma, beta, split)
    ops.layernorm(x, gamma, beta, y32)
    assert torch.equal(_bits(split[:, :c]), _bits(plain))
    ref = F.layer_norm(x.double(), (c,), gamma.double(), beta.double(), 1e-5)
    got = split[:, :c].double() + split[:, c:].double()
    e_split, e_f32, e_f16 = rel_l2(got, ref), rel_l2(y32, ref), rel_l2(plain, ref)
    print(f"\nlayernorm rows={rows} c={c}: hi+lo {e_split:.3e}, f32 kernel {e_f32:.3e}, f16 kernel {e_f16:.3e}")
    assert e_split <= 2 * e_f32


@pytest.mark.parametrize("c1,c2,rows", [(64, 0, 1000), (320, 0, 77), (64, 320, 301)])
def test_cast_concat_split(dev, c1, c2, rows):
    from seva import ops
    g = torch.Generator().manual_seed(c1 + c2)
    # magnitudes from f16-subnormal low parts to values near the top of the f16 range
    x1 = (torch.randn(rows, c1, generator=g) * torch.exp2(torch.randint(-12, 14, (rows, 1), generator=g).float())).to(dev)
    x2 = (torch.randn(rows, c2, generator=g) * 3).to(dev) if c2 else None
    out = torch.full((rows, 2 * (c1 + c2)), float("nan"), dtype=F16, device=dev)
    ops.cast_concat_f16_split(x1, x2, out)
    v = torch.cat([x1, x2], 1) if c2 else x1
    hi, lo = _hilo(v)
    assert torch.equal(_bits(out[:, : c1 + c2]), _bits(hi)) and torch.equal(_bits(out[:, c1 + c2:]), _bits(lo))
    plain = torch.empty((rows, c1 + c2), dtype=F16, device=dev)
    ops.cast_concat_f16(x1, x2, plain)
    assert torch.equal(_bits(plain), _bits(hi))


GUARD = 8
SENTINEL = 0x7BFF  # f16 65504


def _guarded(M, width, dev):
    t = torch.full((M, width + GUARD), 65504.0, dtype=F16, device=dev)
    return t


@pytest.mark.parametrize("N", [64, 320])
@pytest.mark.parametrize("M", [1, 127, 128, 129])
def test_gemm_split_out_plain_is_exact_on_integers(dev, M, N):
    """out = a @ w^T + bias with integer a, even integer w and odd integer bias: every result is an odd integer below 2^16 (most need more
    than the 11 bits of an f16), so hi + lo must reproduce it exactly; the fp32 output beside it too."""
    from seva import ops
    g = torch.Generator().manual_seed(M * 1000 + N)
    K = 128
    a = torch.randint(-3, 4, (M, K), generator=g).float()
    w = 2 * torch.randint(-1, 2, (N, K), generator=g).float()
    bias = (2 * torch.randint(600, 30000, (N,), generator=g) + 1).float()  # odd, 1201 .. 59999; |a @ w^T| <= 768
    exact = a.double() @ w.double().T + bias.double()
    assert float(exact.min()) > 0 and float(exact.max()) < 65504 and bool((exact % 2 == 1).all())
    out16, out32 = _guarded(M, 2 * N, dev), torch.empty((M, N), dtype=F32, device=dev)
    ops.gemm_split_out(a.half().to(dev), w.half().to(dev), bias=bias.to(dev), out_f16=out16, out_f32=out32)
    hi, lo = out16[:, :N].cpu(), out16[:, N:2 * N].cpu()
    assert torch.equal(hi.double() + lo.double(), exact)
    assert torch.equal(_bits(hi), _bits(exact.float().half())) and bool((lo != 0).any())
    assert torch.equal(out32.cpu().double(), exact)
    assert bool((_bits(out16[:, 2 * N:]) == SENTINEL).all())  # guard columns beyond 2N untouched


@pytest.mark.parametrize("N", [64, 320])
@pytest.mark.parametrize("M", [1, 127, 128, 129])
def test_gemm_split_out_geglu_is_exact_on_integers(dev, M, N):
    """GEGLU epilogue, N hidden features (2N interleaved weight rows): value v odd in [17, 825], gate g an odd integer >= 9, where
    gelu(g) == g to fp64 precision and in the kernel's erf approximation alike (erf(g / sqrt 2) rounds to 1): v * g is an odd integer
    below 2^16."""
    from seva import ops
    from seva._engine import interleave_geglu
    g_ = torch.Generator().manual_seed(M * 1000 + N + 1)
    K = 128
    a = torch.randint(0, 4, (M, K), generator=g_).float()
    wv = 2 * torch.randint(-1, 2, (N, K), generator=g_).float()
    wv[:, 64:] = 0                                   # |a @ wv^T| <= 384
    wg = torch.zeros(N, K)
    wg[:, 64:72] = 2 * torch.randint(0, 2, (N, 8), generator=g_).float()  # a @ wg^T even, <= 48
    bv = (2 * torch.randint(200, 221, (N,), generator=g_) + 1).float()    # odd, 401 .. 441
    bg = (2 * torch.randint(4, 7, (N,), generator=g_) + 1).float()        # 9, 11, 13
    wi, bi = interleave_geglu(torch.cat([wv, wg], 0), torch.cat([bv, bg], 0))
    v = a.double() @ wv.double().T + bv.double()
    gate = a.double() @ wg.double().T + bg.double()
    exact = v * F.gelu(gate)
    assert torch.equal(exact, v * gate) and float(exact.min()) > 0 and float(exact.max()) < 65504 and bool((exact % 2 == 1).all())
    out16 = _guarded(M, 2 * N, dev)
    ops.gemm_split_out(a.half().to(dev), wi.half().to(dev), bias=bi.to(dev), out_f16=out16, geglu=True)
    hi, lo = out16[:, :N].cpu(), out16[:, N:2 * N].cpu()
    assert torch.equal(hi.double() + lo.double(), exact)
    assert torch.equal(_bits(hi), _bits(exact.float().half())) and bool((lo != 0).any())
    assert bool((_bits(out16[:, 2 * N:]) == SENTINEL).all())


def test_gemm_split_out_refuses_what_it_does_not_do(dev):
    from seva import ops
    from seva._native import SevaNativeError
    a, w = torch.zeros((64, 64), dtype=F16, device=dev), torch.zeros((64, 64), dtype=F16, device=dev)
    o32 = torch.empty((64, 64), dtype=F32, device=dev)
    with pytest.raises(SevaNativeError, match="ldo16"):  # a pitch that cannot hold [hi | lo]
        ops.gemm_split_out(a, w, out_f16=torch.empty((64, 64), dtype=F16, device=dev))
    with pytest.raises(ValueError):
        ops.gemm_split_out(a, w, out_f32=o32)  # no out_f16
    with pytest.raises(ValueError):
        ops.gemm_split_out(a, w, out_f16=torch.empty((64, 128), dtype=F16, device=dev), out_f32=o32,
                           ch_stats=torch.empty(ops.channel_stats_shape(64, 64), dtype=F32, device=dev))
    with pytest.raises(ValueError):
        ops.gemm_split_out(a.view(torch.uint8), w.view(torch.uint8), w_exp=torch.zeros(64, dtype=torch.uint8, device=dev),
                           out_f16=torch.empty((64, 128), dtype=F16, device=dev))


# ------------------------------------------------------------------------------------- a split operand through the consumers
def _split_ints(shape, g, hi_lim):
    """Integers that need more than 11 bits, below 2^15 (and below `hi_lim`, so that every partial sum of the test stays exact in fp32)."""
    v = torch.randint(2049, hi_lim, shape, generator=g).float() * (2 * torch.randint(0, 2, shape, generator=g).float() - 1)
    hi, lo = _hilo(v)
    assert bool((lo != 0).any())
    return v, torch.cat([hi, lo], -1)


def test_split_operand_through_gemm_is_exact(dev):
    from seva import ops
    from seva._engine import dup_k
    g = torch.Generator().manual_seed(3)
    M, c, N = 200, 320, 320
    v, a = _split_ints((M, c), g, 32768)  # |sum| <= 320 * 32767 < 2^24
    w = torch.randint(-1, 2, (N, c), generator=g).float()
    out = torch.empty((M, N), dtype=F32, device=dev)
    ops.gemm(a.to(dev), dup_k(w.half()).to(dev), out_f32=out, alg_k=c)
    assert torch.equal(out.cpu().double(), v.double() @ w.double().T)


@pytest.mark.parametrize("hw,cout", [(8, 128), (9, 160)])
def test_split_operand_through_conv3x3_is_exact(dev, hw, cout):
    from seva import ops
    from seva._engine import pack_conv3x3
    g = torch.Generator().manual_seed(hw)
    n, c = 2, 64
    v, x = _split_ints((n, hw, hw, c), g, 16384)  # |sum| <= 576 * 16383 < 2^24
    w = torch.randint(-1, 2, (cout, c, 3, 3), generator=g).float()
    out = torch.empty((n, hw * hw, cout), dtype=F32, device=dev)
    ops.conv3x3(x.to(dev), pack_conv3x3(torch.cat([w, w], 1)).to(dev), out_f32=out, alg_k=9 * c)
    ref = F.conv2d(v.double().permute(0, 3, 1, 2), w.double(), None, padding=1).permute(0, 2, 3, 1).reshape(n, hw * hw, cout)
    assert torch.equal(out.cpu().double(), ref)


# -------------------------------------------------------------------------------------------------------- the network under `all`
def _build(tag, dev, split="all"):
    from seva import synthetic as synth
    from seva.model import Seva, SevaParams
    from test_split_operands_cpu import _shapes
    params = SevaParams() if tag == "full" else SevaParams(model_channels=64)
    sd = synth.synth_state_dict(_shapes(tag), 0)
    with torch.device("meta"):
        net = Seva(params)
    net.load_state_dict(sd, strict=True, assign=True)
    net = net.to(dev).eval()
    return net.set_precision("f16", split=split)


@pytest.fixture(scope="module")
def tiny_all(dev):
    return _build("tiny", dev)


def _forward_err(net, dev, name):
    from seva.model import SGMWrapper
    g = load_golden(name)
    T = int(g["T"])
    c = {k: g[k].to(dev) for k in ("crossattn", "concat", "dense_vector")}
    y = SGMWrapper(net)(g["x"].to(dev), g["t"].to(dev), c, num_frames=T).cpu()
    return rel_l2(y, g["y"]), max(rel_l2(y[i], g["y"][i]) for i in range(y.shape[0]))


def test_tiny_forward_under_all_vs_golden(dev, tiny_all):
    from seva._engine import SPLIT_ALL
    assert tiny_all.engine().split == SPLIT_ALL
    err, worst = _forward_err(tiny_all, dev, "g3_tiny_forward")
    print(f"\ntiny forward (T=4, 16x16) under split=all vs reference golden: rel-L2 {err:.3e}, worst latent {worst:.3e} "
          f"[predicted {PRED_TINY:.3e}, bound {1.5 * PRED_TINY:.3e}]")
    assert err <= 1.5 * PRED_TINY


def test_full_forward_under_all_vs_golden(dev):
    """BASELINE config 1 (T=4, 32x32 latent, CFG batch 8), 1.3 B parameters.  Without the mode (`all` not understood) the forward
    measures the f16 floor, about 8e-4."""
    net = _build("full", dev)
    err, worst = _forward_err(net, dev, "g4_full_forward")
    print(f"\n1.3B forward (config 1) under split=all vs reference golden: rel-L2 {err:.3e}, worst latent {worst:.3e} "
          f"[predicted {PRED_CONFIG1:.3e}, bound {1.5 * PRED_CONFIG1:.3e}]")
    assert err <= 1.5 * PRED_CONFIG1


def test_batch_invariance_under_all(dev, tiny_all):
    """Frame 0 of a T = 2 call, alone (n = 2) and with a second scene behind it (n = 4): the same bits."""
    eng = tiny_all.engine()
    g = torch.Generator().manual_seed(41)
    T, h, w, n = 2, 16, 16, 4
    x, t = torch.randn(n, 11, h, w, generator=g).to(dev), torch.randint(0, 1000, (n,), generator=g).to(dev)
    y, dense = torch.randn(n, 1, 1024, generator=g).to(dev), torch.randn(n, 6, h, w, generator=g).to(dev)
    big = eng.forward(x, None, t, y, dense, T).clone()
    small = eng.forward(x[:2].contiguous(), None, t[:2].contiguous(), y[:2].contiguous(), dense[:2].contiguous(), T).clone()
    assert torch.isfinite(big).all() and torch.equal(small[0], big[0]) and torch.equal(small, big[:2])


def test_whole_step_graph_equals_eager_under_all(dev, tiny_all, monkeypatch):
    """6-step loop with the whole sampler step captured into one hipGraph (step 1) and replayed (steps 2-5) against the all-eager loop:
    bit for bit, with every split producer and doubled-K consumer inside the capture."""
    from seva import sampling as S
    from test_model_gpu import _loop
    T, hw, steps = 4, 16, 6
    g = torch.Generator().manual_seed(5)
    eps = [torch.randn(T, 4, hw, hw, generator=g) for _ in range(steps)]
    monkeypatch.setenv("SEVA_STEPGRAPH", "0")
    monkeypatch.setenv("SEVA_HIPGRAPH", "0")
    ref, s0 = _loop(tiny_all, dev, T, hw, steps, eps, S.MultiviewCFG(1.2))
    assert s0._step_graphs.captures == 0
    monkeypatch.setenv("SEVA_STEPGRAPH", "1")
    monkeypatch.setenv("SEVA_HIPGRAPH", "1")
    got, s1 = _loop(tiny_all, dev, T, hw, steps, eps, S.MultiviewCFG(1.2))
    assert s1._step_graphs.captures == 1 and s1._step_graphs.graph.replays == steps - 1
    assert torch.equal(got, ref)
