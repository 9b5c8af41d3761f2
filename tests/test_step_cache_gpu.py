"""Opt-in reuse of deep UNet features across sampler steps, on the device (tiny network): a shallow network call on the inputs
of the last full call returns the full call's bits, eagerly and replayed from its own hipGraph, in f16 and in the fp8 mode; on
other inputs it is the CPU oracle composed the same way; and a sampler run with `cache_interval=2` is, bit for bit, the loop
written out here, with whole-step graphs on or off, on the first trajectory and on the second."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import load_golden, rel_l2  # noqa: E402
from test_model_gpu import NET_TOL, _build, dev, tiny  # noqa: E402,F401  (module-scoped fixtures, not copied into a conftest)
from test_step_cache_cpu import _entry_name, _inputs, _oracle_shallow  # noqa: E402

T_TINY, HW_TINY, STEPS = 4, 16, 6  # the sizes of `churn_cases.TINY`


def _to(args, dev):
    return tuple(a.to(dev) if isinstance(a, torch.Tensor) else a for a in args)


def _golden_inputs():
    g = load_golden("g3_tiny_forward")
    return g["x"], g["concat"], g["t"], g["crossattn"], g["dense_vector"], int(g["T"])


def _same_inputs(eng, args):
    """Full then shallow on `args`, eagerly and through `forward_graphed` (capture, then replay): always the full call's bits, and
    the reused tensor keeps its own."""
    full = eng.forward(*args).clone()
    assert torch.isfinite(full).all()
    for L in (1, 2, 3):
        entry = eng._shallow_entries[eng._last_full][L]
        buf, stats = entry.t, entry.stats
        # (the arena is shared by every shape this engine has run: one buffer of that name per shape)
        assert sum(t is buf for k, t in eng.arena.bufs.items() if k[0] == _entry_name(eng, L)) == 1
        before, st_before = buf.clone(), None if stats is None else stats.clone()
        assert torch.equal(eng.forward(*args, shallow_levels=L), full), L
        assert torch.equal(buf, before) and (stats is None or torch.equal(stats, st_before))
    graphs = len(eng._graphs)
    assert torch.equal(eng.forward_graphed(*args), full)
    for L in (1, 2, 3):
        for _ in range(2):  # the capturing call, then a replay
            assert torch.equal(eng.forward_graphed(*args, shallow_levels=L), full), L
    assert len(eng._graphs) - graphs in (3, 4)  # one graph per depth (and the full call's, unless an earlier test made it)
    return full


@pytest.mark.parametrize("case", ["g3_tiny_forward", "T3_8x24", "T2_32x32_stats2"])
def test_shallow_call_on_the_same_inputs_is_the_full_call(dev, tiny, case):
    net, _ = tiny
    eng = net.engine()
    args = {"g3_tiny_forward": _golden_inputs, "T3_8x24": lambda: _inputs(3, 8, 24, 5), "T2_32x32_stats2": lambda: _inputs(2, 32, 32, 7)}[case]()
    keep = eng.gn_fused_stats
    try:
        if case == "T2_32x32_stats2":
            eng.gn_fused_stats = 2
        _same_inputs(eng, _to(args, dev))
        if case == "T2_32x32_stats2":
            assert any(e.stats is not None for e in eng._shallow_entries[eng._last_full].values())  # statistics did travel
    finally:
        eng.gn_fused_stats = keep


def test_shallow_call_in_the_fp8_mode(dev):
    net, _ = _build("tiny", dev)
    net.set_precision("fp8")
    eng = net.engine()
    assert eng.fp8 and any(k.endswith("8e") for k in eng.W)
    _same_inputs(eng, _to(_inputs(4, 32, 32, 11), dev))


def test_graphed_shallow_call_passes_the_guard_before_every_replay(dev, tiny):
    from seva._native import SevaNativeError
    net, _ = tiny
    eng = net.engine()
    a, b = _to(_inputs(2, 8, 8, 1), dev), _to(_inputs(3, 8, 8, 2), dev)
    full = eng.forward_graphed(*a).clone()
    assert torch.equal(eng.forward_graphed(*a, shallow_levels=1), full)
    eng.forward_graphed(*b)
    with pytest.raises(SevaNativeError, match="num_frames 3 -> 2"):
        eng.forward_graphed(*a, shallow_levels=1)
    eng.forward_graphed(*a)  # a replay of the full graph refills what the shallow graph reads
    assert torch.equal(eng.forward_graphed(*a, shallow_levels=1), full)


@pytest.mark.parametrize("L", [1, 2, 3])
def test_shallow_call_on_other_inputs_vs_the_oracle(dev, tiny, L):
    """Full at (x1, t1, c1), shallow at (x2, t2, c2), against the CPU oracle composed the same way from the trace of its own full
    run at (x1, t1, c1); held to NET_TOL.  And it is not the full call at (x2, t2, c2)."""
    from oracle import seva_ref as O
    net, sd = tiny
    eng = net.engine()
    x1, c1, t1, y1, d1, T = _golden_inputs()
    g = torch.Generator().manual_seed(91)
    x2, c2, y2, d2 = (torch.randn(v.shape, generator=g) for v in (x1, c1, y1, d1))
    t2 = torch.randint(0, 1000, t1.shape, generator=g)
    one, two = _to((x1, c1, t1, y1, d1, T), dev), _to((x2, c2, t2, y2, d2, T), dev)
    full2 = eng.forward(*two).cpu()
    trace = {}
    O.seva_forward(sd, torch.cat([x1, c1], 1), t1, y1, d1, T, trace=trace)
    eng.forward(*one)
    got = eng.forward(*two, shallow_levels=L).cpu()
    ref = _oracle_shallow(sd, torch.cat([x2, c2], 1), t2, y2, d2, T, L, trace)
    err = rel_l2(got, ref)
    full_err = rel_l2(full2, O.seva_forward(sd, torch.cat([x2, c2], 1), t2, y2, d2, T))
    away = rel_l2(got, full2)
    print(f"\nL={L}: shallow call vs composed oracle rel-L2 {err:.3e}; the full call's own error at (x2, t2, c2) {full_err:.3e}; "
          f"shallow vs full at (x2, t2, c2) {away:.3e}")
    assert err < NET_TOL
    assert away > NET_TOL


# ------------------------------------------------------------------------------------------------ sampler
def _scene(dev):
    from seva import sampling as S
    from seva import synthetic as synth
    sc = synth.synth_scene(T_TINY, (HW_TINY, HW_TINY), (0,), seed=23)
    cond = {k: v.to(dev) for k, v in sc["cond"].items()}
    uc = {k: v.to(dev) for k, v in sc["uc"].items()}
    kw = dict(c2w=sc["c2w"].to(dev), K=sc["K"].to(dev), input_frame_mask=sc["input_frame_mask"].to(dev))
    disc = S.DDPMDiscretization()
    return sc["noise"], cond, uc, kw, disc, S.DiscreteDenoiser(disc, num_idx=1000, device=dev)


def _eps():
    g = torch.Generator().manual_seed(5)
    return [torch.randn(T_TINY, 4, HW_TINY, HW_TINY, generator=g) for _ in range(STEPS)]


def _runner(net, dev, solver, N, L):
    """The same sampler, cond objects and denoiser callable for every call of run()"""
    from seva import sampling as S
    from seva.model import SGMWrapper
    noise, cond, uc, kw, disc, den = _scene(dev)
    sampler = S.EulerEDMSampler(disc, S.MultiviewCFG(1.2), num_steps=STEPS, verbose=False, device=dev, s_churn=0.0, solver=solver,
                                cache_interval=N, cache_levels=L)
    wrap = SGMWrapper(net)
    denoiser = lambda x, s, c: den(wrap, x, s, c, num_frames=T_TINY)  # noqa: E731
    eps = _eps()

    def run():
        it = iter(eps)
        sampler.noise_fn = lambda x: next(it).to(x.device)
        return sampler(denoiser, noise.to(dev), scale=2.0, cond=cond, uc=uc, verbose=False, **kw)

    return run, sampler


def _written_out(net, dev, solver, N, L):
    """The trajectory as a plain loop: `engine.forward(..., shallow_levels=...)` under the schedule, the product's denoiser
    scaling around it, and the fused update kernel of the solver, called here."""
    from seva import ops
    from seva import sampling as S
    noise, cond, uc, kw, disc, den = _scene(dev)
    guider, eng, eps = S.MultiviewCFG(1.2), net.engine(), _eps()
    sigmas = disc(STEPS, device=dev)
    x = noise.to(dev).clone()
    s_in = x.new_ones([T_TINY])
    ops.scale_rows(x, torch.sqrt(1.0 + sigmas[0] ** 2.0).expand(T_TINY).contiguous(), x)
    hist, prev = torch.zeros_like(x), torch.zeros_like(s_in)
    for i in range(STEPS):
        level = 0 if i % N == 0 or i == STEPS - 1 else L
        network = lambda xin, t, c: eng.forward(xin, c["concat"], t, c["crossattn"], c["dense_vector"], T_TINY, shallow_levels=level)  # noqa: E731
        sigma, nxt = s_in * sigmas[i], s_in * sigmas[i + 1]
        out = torch.empty_like(x)
        if solver == "euler":
            sigma_hat = sigma * (0.0 + 1.0) + 1e-6
            x_in = torch.empty_like(x)
            ops.add_noise(x, eps[i].to(dev), ((sigma_hat**2 - sigma**2) ** 0.5 * 1.0).contiguous(), x_in)
        else:
            sigma_hat, x_in = sigma, x
        den2 = den(network, *guider.prepare_inputs(x_in, sigma_hat, cond, uc))
        fs = S._scale_vector(guider.frame_scale(den2, sigma_hat, 2.0, **kw), T_TINY, x.device)
        if solver == "euler":
            ops.cfg_euler(x_in, den2, fs, sigma_hat, nxt - sigma_hat, out)
        else:
            a, b, c = S.EulerEDMSampler.multistep_coefficients(sigma, nxt, prev)
            ops.cfg_multistep(x, den2, fs, hist, a, b, c, out, hist)
            prev = sigma
        x = out
    return x


@pytest.mark.parametrize("solver", ["euler", "dpmpp2m"])
def test_sampler_run_is_the_loop_written_out(dev, tiny, solver, monkeypatch):
    net, _ = tiny
    N, L = 2, 1
    for name in ("SEVA_SOLVER", "SEVA_CACHE_INTERVAL", "SEVA_CACHE_LEVELS"):
        monkeypatch.delenv(name, raising=False)
    want = _written_out(net, dev, solver, N, L)
    assert torch.isfinite(want).all()
    monkeypatch.setenv("SEVA_STEPGRAPH", "0")
    run0, s0 = _runner(net, dev, solver, N, L)
    got0 = run0()
    assert s0._step_graphs.captures == 0 and torch.equal(got0, want)
    monkeypatch.setenv("SEVA_STEPGRAPH", "1")
    run1, s1 = _runner(net, dev, solver, N, L)
    got1 = run1()
    cache = s1._step_graphs
    # full steps 0 2 4 5: warm-up, capture + replay, 2 replays; shallow steps 1 3: warm-up, capture + replay
    assert torch.equal(got1, want) and not cache.disabled and cache.captures == 2
    assert (cache.entries[0].graph.replays, cache.entries[L].graph.replays) == (3, 1)
    # a second trajectory through the same sampler: both graphs serve it from the first step on
    assert torch.equal(run1(), want)
    assert cache.captures == 2 and (cache.entries[0].graph.replays, cache.entries[L].graph.replays) == (3 + 4, 1 + 2)
    assert torch.equal(run0(), want)
    # the mode changes the result (the test would pass on a sampler that ignored it otherwise)
    plain, _ = _runner(net, dev, solver, 0, L)
    assert not torch.equal(plain(), want)
