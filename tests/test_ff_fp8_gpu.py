"""e4m3 fused feed-forward (seva_ff_fused_fp8), the opt-in `ff="fp8"` sub-option of the fp8 mode: bit for bit against fp64 on
integer data for every C, the LayerNorm prologue against the torch emulation and against the unquantised feed-forward, against the
two-kernel e4m3 chain on the same weights, row independence at the step's shape, the 1.3B network at the headline shape and the
whole-step hipGraph.  Restatements and emulation: tests/test_ff_fp8_cpu.py."""
import pytest
import torch

from conftest import rel_l2
from test_ff_fp8_cpu import STEP, feature_of, ff_fp32, ff_fp8_reference, layernorm_e4m3, random_ff

pytestmark = pytest.mark.gpu
CS = (64, 128, 256, 320)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from seva import _native
    _native.load()
    return torch.device("cuda:0")


def _to8(x: torch.Tensor) -> torch.Tensor:
    return x.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)


def _integer_problem(c: int, M: int, seed: int):
    """Integer-valued operands on which every step of the kernel is exact: a in {-1, 0, 1}; value rows of W1 with one non-zero
    +-2^s (s in -2..0: v in {0, +-1/4, +-1/2, +-1}); gate rows with four +-1 and gate bias 12 (g in [8, 16]: gelu(g) = g in fp32,
    and v g is exact in e4m3); W2 small integers times random power-of-two row scales; integer b2 and residual.  The stored
    W1 bytes carry random power-of-two row scales too (q = w 2^-e)."""
    g = torch.Generator().manual_seed(seed)
    kp = (c + 127) // 128 * 128
    a = torch.randint(-1, 2, (M, c), generator=g).float()
    rows = torch.arange(8 * c)
    is_gate = (rows % 64) >= 32
    # value rows: one non-zero +-2^s, stored q = +-1 with e = s
    w1 = torch.zeros(8 * c, c)
    e1 = -torch.randint(0, 3, (8 * c,), generator=g).float()
    sign = torch.randint(0, 2, (8 * c, 4), generator=g).float() * 2 - 1
    kv = torch.randint(0, c, (8 * c,), generator=g)
    kg = torch.argsort(torch.rand(8 * c, c, generator=g), dim=1)[:, :4]
    for r in range(8 * c):
        if is_gate[r]:
            w1[r, kg[r]] = sign[r]  # stored q = +-2^-e in {1, 2, 4}
        else:
            w1[r, kv[r]] = sign[r, 0] * 2.0 ** float(e1[r])
    q1 = w1 * torch.exp2(-e1)[:, None]
    b1 = torch.where(is_gate, torch.full((8 * c,), 12.0), torch.zeros(8 * c))
    q2 = torch.randint(-2, 3, (c, 4 * c), generator=g).float()
    e2 = torch.randint(-2, 2, (c,), generator=g).float()
    w2 = q2 * torch.exp2(e2)[:, None]
    b2 = torch.randint(-4, 5, (c,), generator=g).float()
    res = torch.randint(-8, 9, (M, c), generator=g).float()
    # stored forms
    w1_8 = torch.zeros(8 * c, kp, dtype=torch.uint8)
    w1_8[:, :c] = _to8(q1)
    w1_exp = (e1 + 127).to(torch.uint8)
    i = torch.arange(4 * c)
    perm = (i // STEP) * STEP + feature_of(i % STEP)
    w2_8 = _to8(q2)[:, perm].contiguous()
    w2_exp = (e2 + 127).to(torch.uint8)
    # a: [M, kp + 16] bytes; the columns >= C hold NaN bytes (the kernel must not read them)
    a8 = torch.full((M, kp + 16), 0x7F, dtype=torch.uint8)
    a8[:, :c] = _to8(a)
    # fp64 reference (gelu(g) = g for g >= 8 in fp32; v g exact in e4m3)
    h = (a.double() @ w1.double().T + b1.double()).view(M, 4 * c // 32, 2, 32)
    v, gt = h[:, :, 0], h[:, :, 1]
    assert (gt >= 8).all() and (gt <= 16).all()
    hid = (v * gt).reshape(M, 4 * c)
    assert torch.equal(hid.float().to(torch.float8_e4m3fn).double(), hid)
    out = hid @ w2.double().T + b2.double()
    return (a8, w1_8, w1_exp, b1, w2_8, w2_exp, b2, res), out


@pytest.mark.parametrize("c", CS)
def test_bit_exact_on_integer_data(dev, c):
    from seva import ops
    for M in (1, 127, 128, 129, 1000, 4097):
        (a8, w1_8, w1_exp, b1, w2_8, w2_exp, b2, res), out = _integer_problem(c, M, seed=c * 7919 + M)
        d = [t.to(dev) for t in (a8, w1_8, w1_exp, b1, w2_8, w2_exp, b2, res)]
        for with_res in (False, True):
            o32 = torch.full((M, c), float("nan"), device=dev)
            o16 = torch.full((M, c + 8), float("nan"), device=dev, dtype=torch.float16)[:, :c]
            ops.ff_fused_fp8(d[0], d[1], d[2], d[3], d[4], d[5], d[6], residual=d[7] if with_res else None,
                             out_f32=o32, out_f16=o16)
            ref = (out + res.double()) if with_res else out
            assert torch.equal(o32.cpu(), ref.float()), (c, M, with_res, rel_l2(o32.cpu(), ref))
            assert torch.equal(o16.cpu(), ref.float().half()), (c, M, with_res)


def test_validation_errors(dev):
    from seva import _native as nv
    from seva import ops
    (a8, w1_8, w1_exp, b1, w2_8, w2_exp, b2, _), _ = _integer_problem(64, 16, seed=1)
    d = [t.to(dev) for t in (a8, w1_8, w1_exp, b1, w2_8, w2_exp, b2)]
    out = torch.empty((16, 64), device=dev)
    lib = nv.load()

    def desc(**kw):
        x = nv.FfDesc()
        x.a, x.w1, x.w1_exp, x.b1, x.w2, x.w2_exp, x.b2 = (t.data_ptr() for t in d)
        x.out_f32, x.M, x.lda, x.ldo32, x.C = out.data_ptr(), 16, d[0].stride(0), 64, 64
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    import ctypes
    s = nv.stream_ptr(dev)
    assert lib.seva_ff_fused_fp8(ctypes.byref(desc()), s) == 0
    for kw, what in (({"C": 96}, "C=96"), ({"w1_exp": None}, "w1_exp"), ({"w2_exp": None}, "w1_exp"),
                     ({"a": None}, "neither"), ({"lda": 72}, "lda"), ({"a": d[0].data_ptr() + 8}, "aligned"),
                     ({"ldo32": 66}, "multiples of 4")):
        assert lib.seva_ff_fused_fp8(ctypes.byref(desc(**kw)), s) < 0, kw
        assert what in lib.seva_last_error().decode(), (kw, lib.seva_last_error())
    torch.cuda.synchronize()
    with pytest.raises(AssertionError):
        ops.ff_fused_fp8(d[0], d[1], d[2], d[3], d[1], d[5], d[6], out_f32=out)  # W2 of the wrong shape


def _ln_problem(c, M, seed):
    from seva import ops
    g = torch.Generator().manual_seed(seed)
    w1i, b1i, w2, b2 = random_ff(c, g)
    x = torch.randn(M, c, generator=g) * 2 + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    res = torch.randn(M, c, generator=g)
    packed = ops.pack_ff_fp8(w1i, w2)
    return (x, gamma, beta, res, w1i, b1i, w2, b2), packed


def _run_ln(dev, x, gamma, beta, res, packed, b1i, b2):
    from seva import ops
    w1_8, w1_exp, w2_8, w2_exp = (t.to(dev) for t in packed)
    out = torch.empty(x.shape, device=dev)
    ops.ff_fused_fp8(None, w1_8, w1_exp, b1i.to(dev), w2_8, w2_exp, b2.to(dev), residual=res.to(dev), out_f32=out,
                     ln_x=x.to(dev), ln_gamma=gamma.to(dev), ln_beta=beta.to(dev))
    return out


@pytest.mark.parametrize("c", CS)
def test_layernorm_path_against_the_emulation_and_fp32(dev, c):
    M = 1500
    (x, gamma, beta, res, w1i, b1i, w2, b2), packed = _ln_problem(c, M, 11 + c)
    out = _run_ln(dev, x, gamma, beta, res, packed, b1i, b2).cpu()
    emu = ff_fp8_reference(layernorm_e4m3(x, gamma, beta), *packed[:2], b1i, *packed[2:], b2, res)
    ref = ff_fp32(x, gamma, beta, w1i, b1i, w2, b2, res)
    err = rel_l2(out.double() - res.double(), emu - res.double())
    err32 = rel_l2(out.double() - res.double(), ref - res.double())
    print(f"\nC={c}: e4m3 fused feed-forward (LayerNorm prologue) vs emulation rel-L2 {err:.3e}; vs unquantised fp32 {err32:.3e}")
    assert torch.isfinite(out).all()
    assert err <= 2e-3  # e4m3 rounding flips at ties (rsqrt, GELU approximation)
    assert 5e-3 < err32 < 8e-2


@pytest.mark.parametrize("c", CS)
def test_against_the_two_kernel_e4m3_chain(dev, c):
    from seva import ops
    M = 2000
    (x, gamma, beta, res, w1i, b1i, w2, b2), packed = _ln_problem(c, M, 23 + c)
    out = _run_ln(dev, x, gamma, beta, res, packed, b1i, b2)
    kp = (c + 127) // 128 * 128
    w1_8, w1_exp, _, w2_exp = (t.to(dev) for t in packed)
    w2n, w2n_exp = ops.quantize_weight_fp8(w2.to(dev))
    assert torch.equal(w2n_exp, w2_exp)
    a8 = torch.zeros((M, kp), dtype=torch.uint8, device=dev)
    ops.layernorm(x.to(dev), gamma.to(dev), beta.to(dev), a8)
    h8 = torch.empty((M, 4 * c), dtype=torch.uint8, device=dev)
    ops.gemm(a8, w1_8, w_exp=w1_exp, bias=b1i.to(dev), out_f8=h8, geglu=True)
    chain = torch.empty((M, c), device=dev)
    ops.gemm(h8, w2n, w_exp=w2n_exp, bias=b2.to(dev), residual=res.to(dev), out_f32=chain)
    err = rel_l2(out.cpu().double() - res.double(), chain.cpu().double() - res.double())
    print(f"\nC={c}: e4m3 fused feed-forward vs the two-kernel e4m3 chain: rel-L2 {err:.3e}")
    assert err <= 1e-3


def test_rows_are_independent_at_the_step_shape(dev):
    """M = 217,728 (T = 21, 72 x 72, both CFG halves): sampled rows (tile edges included) equal the same rows launched alone"""
    M, c = 217728, 320
    (x, gamma, beta, res, w1i, b1i, w2, b2), packed = _ln_problem(c, M, 5)
    full = _run_ln(dev, x, gamma, beta, res, packed, b1i, b2)
    g = torch.Generator().manual_seed(9)
    rows = torch.cat([torch.tensor([0, 1, 127, 128, 129, 255, 256, M - 129, M - 128, M - 1]),
                      torch.randint(0, M, (300,), generator=g)])
    alone = _run_ln(dev, x[rows].contiguous(), gamma, beta, res[rows].contiguous(), packed, b1i, b2)
    assert torch.isfinite(full).all()
    assert torch.equal(full[rows.to(dev)], alone)


def test_fp8_feed_forward_forward_at_the_headline_shape_vs_reference(dev, monkeypatch):
    """fp8 mode + ff="fp8", ONE 1.3B network call at T=21, 576x576 (B=42) against the reference's own output, beside the plain fp8
    mode.  Bounded like the fp8 mode (< 6e-2 overall, < 1e-1 per latent); fp8 with an explicit ff="f16" equals the fp8 default."""
    import os
    from conftest import GOLD, load_golden
    from test_headline_gpu import FORWARD_SEEDS, _wrapper_inputs
    from test_model_gpu import _build
    from seva.model import SGMWrapper
    if not os.path.exists(os.path.join(GOLD, "g9_T21_forward.npz")):
        pytest.skip("g9_T21_forward.npz not generated")
    monkeypatch.delenv("SEVA_FP8_FF", raising=False)
    g = load_golden("g9_T21_forward")
    T = 21
    net, _ = _build("full", dev)
    x, t, c = _wrapper_inputs(T, FORWARD_SEEDS[T])
    run = lambda: SGMWrapper(net)(x.to(dev), t.to(dev), {k: v.to(dev) for k, v in c.items()}, num_frames=T).cpu()  # noqa: E731
    net.set_precision("fp8")
    y8 = run()
    net.set_precision("fp8", ff="f16")
    y8e = run()
    net.set_precision("fp8", ff="fp8")
    y = run()
    eng = net.engine()
    assert eng.ff8 and sum(k.endswith(".w1f8") for k in eng.W) == 15
    ref = g["y"]
    err, err8 = rel_l2(y, ref), rel_l2(y8, ref)
    per = [rel_l2(y[i], ref[i]) for i in range(y.shape[0])]
    print(f"\nfp8 mode + fp8 feed-forward, 1.3B forward T=21 72x72 (B=42) vs REFERENCE: rel-L2 {err:.3e}; per latent max "
          f"{max(per):.3e} (plain fp8 mode: {err8:.3e})")
    assert torch.equal(y8e, y8)
    assert torch.isfinite(y).all() and not torch.equal(y, y8)
    assert 1e-3 < err < 6e-2 and max(per) < 1e-1


def test_whole_step_graph_equals_eager_in_the_fp8_feed_forward_mode(dev, monkeypatch):
    """tiny network (its C = 64 feed-forwards on the e4m3 kernel, with fp8 attention too), 4-step loop: whole-step hipGraph replay
    against the all-eager loop, bit for bit"""
    from test_model_gpu import _build, _loop
    net, _ = _build("tiny", dev)
    net.set_precision("fp8", attention="fp8", ff="fp8")
    T, hw, steps = 4, 48, 4
    g = torch.Generator().manual_seed(5)
    eps = [torch.randn(T, 4, hw, hw, generator=g) for _ in range(steps)]
    monkeypatch.setenv("SEVA_STEPGRAPH", "0")
    monkeypatch.setenv("SEVA_HIPGRAPH", "0")
    ref, s0 = _loop(net, dev, T, hw, steps, eps)
    assert net.engine().ff8 and s0._step_graphs.captures == 0
    monkeypatch.setenv("SEVA_STEPGRAPH", "1")
    monkeypatch.setenv("SEVA_HIPGRAPH", "1")
    got, s1 = _loop(net, dev, T, hw, steps, eps)
    assert s1._step_graphs.captures == 1
    assert torch.isfinite(got).all() and torch.equal(got, ref)
