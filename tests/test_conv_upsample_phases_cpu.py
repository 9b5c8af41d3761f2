"""Host side of the phase-decomposed Upsample conv (`ops.conv3x3_up_phases`; reference seva/modules/layers.py:35-46): the weight
combination `seva._engine.combine_up_phases`, checked by running the four 2x2 convs on the SOURCE image in torch and interleaving
them, and the engine's choice of path.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import fake_ops
from conftest import rel_l2
from test_engine_host_logic import _cpu_engine


def _phase_conv(x, w4, bias=None):
    """x [n, cin, h, w], w4 [4, cout, 4 cin] (phase 2 py + px, K ordered (a, b, ci)) -> [n, cout, 2h, 2w]: tap (a, b) of phase
    (py, px) sits at source offset (a + py - 1, b + px - 1); zero border."""
    n, cin, h, w = x.shape
    cout = w4.shape[1]
    xp = F.pad(x, (1, 1, 1, 1))
    out = x.new_zeros((n, cout, 2 * h, 2 * w))
    for py in range(2):
        for px in range(2):
            k = w4[2 * py + px].to(x.dtype).reshape(cout, 2, 2, cin).permute(0, 3, 1, 2)
            out[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + h + 1, px:px + w + 1], k)
    return out if bias is None else out + bias[None, :, None, None]


def _combine64(w):
    """The combination without the final f16 rounding (fp64), from the table in combine_up_phases' docstring."""
    from seva._engine import combine_up_phases
    return combine_up_phases(w, dtype=torch.float64)


@pytest.mark.parametrize("n,cin,cout,h,w", [(2, 8, 6, 7, 5), (1, 4, 4, 5, 8), (3, 16, 8, 1, 1), (1, 3, 5, 2, 9), (2, 8, 8, 16, 24)])
def test_four_phase_convs_equal_upsample_then_conv(n, cin, cout, h, w):
    g = torch.Generator().manual_seed(n * 100 + h)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
    bias = torch.randn(cout, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt, bias, padding=1)
    w4 = _combine64(wt)
    assert w4.dtype == torch.float64 and w4.shape == (4, cout, 4 * cin)
    got = _phase_conv(x, w4, bias)
    assert float((got - ref).abs().max()) < 1e-9


def test_combination_is_bit_exact_on_integers_and_rounds_once():
    from seva._engine import combine_up_phases
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-3, 4, (2, 16, 7, 5), generator=g).float()
    wt = torch.randint(-2, 3, (12, 16, 3, 3), generator=g).float()
    w4 = combine_up_phases(wt)
    assert w4.dtype == torch.float16 and w4.shape == (4, 12, 64) and w4.is_contiguous()
    assert float(w4.abs().max()) <= 8.0
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt, padding=1)
    assert torch.equal(_phase_conv(x, w4.float()), ref)
    # one rounding: the f16 weights are the fp64 sums of the fp32 weights rounded once -- not sums of f16-rounded weights
    wr = torch.randn(8, 8, 3, 3, generator=g) * 0.05
    assert torch.equal(combine_up_phases(wr), _combine64(wr).to(torch.float16))
    twice = _combine64(wr.half().float()).to(torch.float16)
    assert not torch.equal(combine_up_phases(wr), twice)
    # the corner phases keep single weights, the centre tap of phase (0, 0) sums four
    w4r = _combine64(wr).reshape(4, 8, 2, 2, 8)
    assert torch.equal(w4r[0, :, 0, 0], wr[:, :, 0, 0].double()) and torch.equal(w4r[3, :, 1, 1], wr[:, :, 2, 2].double())
    assert torch.allclose(w4r[0, :, 1, 1], wr[:, :, 1:, 1:].double().sum((2, 3)), atol=0, rtol=1e-15)
    assert torch.allclose(w4r[1, :, 0, 0], wr[:, :, 0, :2].double().sum(2), atol=0, rtol=1e-15)


def test_engine_packs_phase_weights_and_keeps_the_nine_tap_call_on_fake_ops(monkeypatch):
    """tests/fake_ops.py has no `conv3x3_up_phases`: the engine must take today's nine-tap call unchanged (and still match the
    reference); with an operator of that name present it takes the phase path, unless SEVA_UPSAMPLE_PHASES=0 -- both decided at
    call time."""
    from oracle import seva_ref as O
    from seva import _engine
    monkeypatch.setattr(_engine, "ops", fake_ops)
    monkeypatch.setattr(_engine, "require_cuda", lambda *a: None)
    monkeypatch.delenv("SEVA_UPSAMPLE_PHASES", raising=False)
    assert not hasattr(fake_ops, "conv3x3_up_phases")
    eng, sd = _cpu_engine()
    ups = [s for s in eng.layout.all_specs() if s.kind == "up"]
    assert ups
    for s in ups:
        w4 = eng.W[s.prefix + ".w4"]
        assert w4.dtype == torch.float16 and w4.shape == (4, s.channels, 4 * s.channels)
        assert torch.equal(w4, _engine.combine_up_phases(sd[s.prefix + ".conv.weight"].float()))
    seen = []
    real = fake_ops.conv3x3
    monkeypatch.setattr(fake_ops, "conv3x3", lambda x, w, **k: (seen.append(bool(k.get("upsample"))), real(x, w, **k))[1])
    g = torch.Generator().manual_seed(11)
    T, h, w = 2, 8, 8
    n = 2 * T
    x, t = torch.randn(n, 11, h, w, generator=g), torch.randint(0, 1000, (n,), generator=g)
    y, dense = torch.randn(n, 1, 1024, generator=g), torch.randn(n, 6, h, w, generator=g)
    ref = O.seva_forward(sd, x, t, y, dense, T)
    out = eng.forward(x, None, t, y, dense, T).clone()
    assert sum(seen) == len(ups) and rel_l2(out, ref) < 2e-3

    # an `ops` that has the operator: emulate it with the four phase convs.  The tiny model's channel counts are not multiples of 160
    # (the kernel's tile width), so the per-sample rule keeps the nine-tap call there; a 320-channel resample takes the phase path
    calls = []

    def up_phases(x16, w4, *, bias=None, out_f32=None, ch_stats=None, alg_k=0):
        assert ch_stats is None
        calls.append(alg_k)
        r = _phase_conv(x16.permute(0, 3, 1, 2).float(), w4.float(), bias)
        out_f32.copy_(r.permute(0, 2, 3, 1).reshape(out_f32.shape))

    monkeypatch.setattr(fake_ops, "conv3x3_up_phases", up_phases, raising=False)
    del seen[:]
    out2 = eng.forward(x, None, t, y, dense, T)
    assert sum(seen) == len(ups) and not calls and torch.equal(out2, out)

    class Spec:
        kind, prefix, channels = "up", "upx", 320

    wt = torch.randn(320, 320, 3, 3, generator=g) * 0.03
    eng.W.update({"upx.w": _engine.pack_conv3x3(wt), "upx.w4": _engine.combine_up_phases(wt), "upx.b": torch.randn(320, generator=g)})
    xs = _engine.Act(torch.randn(2, 6 * 4, 320, generator=g), 2, 6, 4)
    del seen[:]
    o = eng._resample(Spec, xs)
    o4 = o.t.clone()
    assert calls == [9 * 320] and not seen and (o.h, o.w) == (12, 8) and o.stats is None
    monkeypatch.setenv("SEVA_UPSAMPLE_PHASES", "0")
    o9 = eng._resample(Spec, xs).t
    assert calls == [9 * 320] and seen == [True]
    assert rel_l2(o4, o9) < 1e-3  # f16 weight rounding only
