"""Opt-in guidance controls of `seva.sampling`, host side: `EulerEDMSampler(guidance_interval=(sigma_lo, sigma_hi),
guidance_rescale=phi)`, SEVA_GUIDANCE_INTERVAL / SEVA_GUIDANCE_RESCALE, `parse_guidance`, the schedule of guided and unguided
steps (alone, under churn, with `cache_interval`, under `cfg_split` on two gloo ranks), the equivalences with the sampler as it
was, the whole-step graph entries of the step kinds (the stand-in graph of tests/test_stepgraph_cpu.py) and the drivers.  The HIP
operators are emulated by tests/fake_ops.py, `ops.cfg_multistep` by tests/test_solver_dpmpp2m_cpu.py and the new `ops.cfg_rescale`
by tests/fake_guidance_ops.py; the network is a recording stand-in behind the sampler's opaque denoiser."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import fake_guidance_ops
from test_pipeline_cpu import _fake_net, _free_port, _patch_cpu, _scene
from test_solver_dpmpp2m_cpu import SCALE, SHAPE, _fake_cfg_multistep, _rows
from test_stepgraph_cpu import FakeStepGraph

INF = float("inf")
STEPS = 10
SIGMAS = (84.9, 48.3, 30.0, 19.8, 13.5, 9.35, 6.34, 4.05, 2.26, 0.90)  # the 10-step schedule, to three digits
INTERVAL = (3.0, 25.0)  # both bounds lie between schedule values: guides steps 3..7
GUIDED = [False, False, False, True, True, True, True, True, False, False]
N = SHAPE[0]
ENV = ("SEVA_SOLVER", "SEVA_CACHE_INTERVAL", "SEVA_CACHE_LEVELS", "SEVA_GUIDANCE_INTERVAL", "SEVA_GUIDANCE_RESCALE")
SOLVERS = [("euler", 0.0), ("euler", 0.5), ("dpmpp2m", 0.0)]


def _install(monkeypatch=None):
    """fake_ops + the two emulated newer operators; main process: through monkeypatch, spawned workers: plain setattr."""
    import seva.ops as ops
    _patch_cpu(monkeypatch)
    put = setattr if monkeypatch is None else monkeypatch.setattr
    put(ops, "cfg_multistep", _fake_cfg_multistep)
    put(ops, "cfg_rescale", fake_guidance_ops.cfg_rescale)


@pytest.fixture
def cpu_sampler(monkeypatch):
    from seva import sampling as S
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    _install(monkeypatch)
    return S


def test_the_schedule_this_file_assumes(cpu_sampler):
    sig = cpu_sampler.DDPMDiscretization()(STEPS)
    assert len(sig) == STEPS + 1 and float(sig[-1]) == 0.0
    for got, want in zip(sig[:-1].tolist(), SIGMAS):
        assert abs(got - want) <= 0.006 * want, (got, want)
    assert [INTERVAL[0] < s <= INTERVAL[1] for s in SIGMAS] == GUIDED


class Net:
    """A stand-in network behind the sampler's opaque denoiser: records the batch and the depth requested for each call.  Each row
    depends on its own inputs alone (the property of the real network that makes a half batch the half of the full batch), the
    conditional and unconditional rows differ through c["vector"], and shallow calls return another function of the inputs."""

    def __init__(self):
        self.batches, self.levels = [], []

    def __call__(self, xx, ss, cc):
        from seva import _native
        L = _native.network_shallow_levels()
        self.batches.append(xx.shape[0])
        self.levels.append(L)
        k = _rows(1.0 / (1.0 + ss * ss), xx)
        mu = (0.3 - 0.5 * cc["vector"][:, 0] + 0.05 * L).view(-1, 1, 1, 1)
        return mu * (1 - k) + xx * k * (1.0 + 0.1 * cc["vector"][:, :1, None, None])


_COND, _UC = {"vector": torch.ones(N, 1)}, {"vector": torch.zeros(N, 1)}  # the same objects for every run (a graph key holds them)


def _cond():
    return _COND, _UC


def _guider(S, calls):
    class Counting(S.VanillaCFG):
        def prepare_inputs(self, x, s, c, uc):
            calls.append(1)
            return super().prepare_inputs(x, s, c, uc)

        def frame_scale(self, x, sigma, scale, **kw):
            calls.append("scale")
            return super().frame_scale(x, sigma, scale, **kw)

    return Counting()


def _sampler(S, solver, churn=0.0, steps=STEPS, cls=None, guider=None, **kw):
    sm = (cls or S.EulerEDMSampler)(S.DDPMDiscretization(), guider or S.VanillaCFG(), num_steps=steps, verbose=False, device="cpu",
                                    solver=solver, s_churn=churn, **kw)
    sm._step_graphs.disabled = True
    return sm


def _trajectory(sm, net, seed=1):
    g = torch.Generator().manual_seed(seed)
    sm.noise_fn = lambda x: torch.randn(x.shape, generator=g)
    x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(100 + seed))
    cond, uc = _cond()
    return sm(net, x, SCALE, cond, uc, verbose=False)


# ------------------------------------------------------------------------------------------------ parsing
def test_parse_guidance():
    from seva.sampling import parse_guidance as P
    assert P(None, None) == (None, 0.0) and P("", "") == (None, 0.0) and P(" ", None) == (None, 0.0)
    assert P((0.3, 5), 0.7) == ((0.3, 5.0), 0.7) and P([0, INF], 0) == ((0.0, INF), 0.0)
    assert P("0.3,5", "0.7") == ((0.3, 5.0), 0.7) and P("0.5, inf", "1") == ((0.5, INF), 1.0) and P("0,1e-3", "0") == ((0.0, 1e-3), 0.0)
    got = P((1, 2), 1)
    assert all(type(v) is float for v in got[0]) and type(got[1]) is float
    for bad in ((5, 0.3), (1, 1), (-1, 5), (0.3,), (0.3, 5, 7), 0.3, "0.3", "0.3;5", "a,b", "0.3,5,7", (None, 5), (True, 5),
                (float("nan"), 5), (0.3, float("nan")), (INF, INF), ((0.3, 5), None), {0.3, 5}):
        with pytest.raises(ValueError):
            P(bad, None)
    for bad in (-0.1, 1.1, "1.5", "phi", float("nan"), True, (0.5,), [0.5]):
        with pytest.raises(ValueError):
            P(None, bad)


def test_arguments_and_environment(cpu_sampler, monkeypatch):
    S = cpu_sampler
    mk = lambda cls=S.EulerEDMSampler, **kw: cls(S.DDPMDiscretization(), S.VanillaCFG(), num_steps=3, device="cpu", **kw)  # noqa: E731
    got = lambda sm: (sm.guidance_interval, sm.guidance_rescale)  # noqa: E731
    assert got(mk()) == (None, 0.0) and got(mk(guidance_interval=(0.3, 5))) == ((0.3, 5.0), 0.0)
    assert got(mk(guidance_rescale=0.7)) == (None, 0.7) and got(mk(S.DPMPP2MSampler, guidance_interval=(0.5, 3), guidance_rescale=1)) == ((0.5, 3.0), 1.0)
    monkeypatch.setenv("SEVA_GUIDANCE_INTERVAL", "0.3,5")
    assert got(mk()) == ((0.3, 5.0), 0.0) and got(mk(S.DPMPP2MSampler)) == ((0.3, 5.0), 0.0)
    monkeypatch.setenv("SEVA_GUIDANCE_RESCALE", "0.7")
    assert got(mk()) == ((0.3, 5.0), 0.7)
    # an explicit argument wins over the variable
    assert got(mk(guidance_interval=(0, INF))) == ((0.0, INF), 0.7) and got(mk(guidance_rescale=0)) == ((0.3, 5.0), 0.0)
    assert got(mk(guidance_interval=(1, 2), guidance_rescale=0.25)) == ((1.0, 2.0), 0.25)
    for name, bad in (("SEVA_GUIDANCE_INTERVAL", "5,0.3"), ("SEVA_GUIDANCE_INTERVAL", "5"), ("SEVA_GUIDANCE_INTERVAL", "lo,hi"),
                      ("SEVA_GUIDANCE_RESCALE", "2"), ("SEVA_GUIDANCE_RESCALE", "-1"), ("SEVA_GUIDANCE_RESCALE", "half")):
        with monkeypatch.context() as mp_:
            mp_.setenv(name, bad)
            with pytest.raises(ValueError):
                mk()
    for kw in (dict(guidance_interval=(5, 0.3)), dict(guidance_interval=3.0), dict(guidance_rescale=1.5), dict(guidance_rescale=True)):
        with pytest.raises(ValueError):
            mk(**kw)
    for name in ("SEVA_GUIDANCE_INTERVAL", "SEVA_GUIDANCE_RESCALE"):
        monkeypatch.setenv(name, "")
    assert got(mk()) == (None, 0.0)


# ------------------------------------------------------------------------------------------------ schedule
@pytest.mark.parametrize("solver,churn", SOLVERS)
def test_schedule(cpu_sampler, solver, churn):
    """The network batch per step, and the guider's part in exactly the guided steps -- the same under churn, whose sigma_hat of
    step 2 (30.0 * 1.041 = 31.3 > 25 anyway) and of step 7 (4.05 * 1.041 = 4.22) stay inside; see `test_churn_...` for a bound
    that sigma_hat does cross."""
    S = cpu_sampler
    net, calls = Net(), []
    out = _trajectory(_sampler(S, solver, churn, guider=_guider(S, calls), guidance_interval=INTERVAL), net)
    assert net.batches == [N, N, N, 2 * N, 2 * N, 2 * N, 2 * N, 2 * N, N, N] == [2 * N if g else N for g in GUIDED]
    assert calls.count(1) == 5 and calls.count("scale") == 5  # prepare_inputs and the scale rule: the five guided steps only
    plain = Net()
    ref = _trajectory(_sampler(S, solver, churn), plain)
    assert plain.batches == [2 * N] * STEPS and not torch.equal(out, ref) and torch.isfinite(out).all()


def test_prepare_inputs_is_called_on_exactly_the_guided_steps(cpu_sampler):
    S = cpu_sampler
    net, at = Net(), []

    class G(S.VanillaCFG):
        def prepare_inputs(self, x, s, c, uc):
            at.append(len(net.batches))  # = the index of the step that is about to call the network
            return super().prepare_inputs(x, s, c, uc)

    _trajectory(_sampler(S, "euler", guider=G(), guidance_interval=INTERVAL), net)
    assert at == [3, 4, 5, 6, 7]


def test_upper_bound_is_inclusive_and_lower_bound_exclusive(cpu_sampler):
    S = cpu_sampler
    sig = S.DDPMDiscretization()(STEPS)
    s3, s7 = float(sig[3]), float(sig[7])  # the fp32 schedule values themselves, as Python doubles
    for interval, want in (((3.0, s3), [3, 4, 5, 6, 7]),          # sigma_hi ON sigma_3: step 3 is guided (<=)
                           ((s7, 25.0), [3, 4, 5, 6]),            # sigma_lo ON sigma_7: step 7 is not (<)
                           ((3.0, float(torch.nextafter(sig[3], sig[4]))), [4, 5, 6, 7]),  # one fp32 ulp below sigma_3
                           # the comparison is made in the sigmas' dtype: a bound within half an fp32 ulp of sigma_3 IS sigma_3 there
                           ((3.0, s3 * (1 - 2.0 ** -26)), [3, 4, 5, 6, 7])):
        net = Net()
        _trajectory(_sampler(S, "euler", guidance_interval=interval), net)
        assert [i for i, b in enumerate(net.batches) if b == 2 * N] == want, interval


def test_churn_does_not_move_a_step_across_a_bound(cpu_sampler):
    """s_churn = 4 gives gamma = 0.4: sigma_hat of step 3 is 19.8 * 1.4 = 27.8 > 25 and of step 8 is 2.26 * 1.4 = 3.17 > 3.  A
    decision on sigma_hat would unguide step 3 and guide step 8; the decision on the schedule's sigma does neither."""
    S = cpu_sampler
    net = Net()
    sm = _sampler(S, "euler", 4.0, guidance_interval=INTERVAL)
    _trajectory(sm, net)
    assert min(sm.s_churn / STEPS, 2 ** 0.5 - 1) == 0.4 and SIGMAS[3] * 1.4 > INTERVAL[1] and SIGMAS[8] * 1.4 > INTERVAL[0]
    assert [b == 2 * N for b in net.batches] == GUIDED


# ------------------------------------------------------------------------------------------------ equivalences
@pytest.mark.parametrize("solver,churn", SOLVERS)
def test_mode_off_is_the_sampler_without_the_arguments(cpu_sampler, monkeypatch, solver, churn):
    S = cpu_sampler
    calls = []

    class Spy(S.EulerEDMSampler):  # the calls `__call__` makes, keyword for keyword
        def sampler_step(self, *a, **k):
            calls.append((len(a), sorted(k)))
            return super().sampler_step(*a, **k)

    def run(**kw):
        del calls[:]
        net = Net()
        return _trajectory(_sampler(S, solver, churn, cls=Spy, **kw), net), net.batches, list(calls)

    ref, batches, ref_calls = run()
    assert batches == [2 * N] * STEPS and ref_calls == [(8, [])] * STEPS  # `sampler_step` never sees the new keyword
    for kw in (dict(guidance_interval=(0, INF), guidance_rescale=0), dict(guidance_interval=(0, INF)), dict(guidance_rescale=0.0),
               dict(guidance_interval=(0.5, 100.0), guidance_rescale=0)):
        out, b, cl = run(**kw)
        assert torch.equal(out, ref) and b == batches and cl == ref_calls, kw
    monkeypatch.setenv("SEVA_GUIDANCE_INTERVAL", "0,inf")
    monkeypatch.setenv("SEVA_GUIDANCE_RESCALE", "0")
    out, b, cl = run()
    assert torch.equal(out, ref) and b == batches and cl == ref_calls
    # and with the interval on, only the unguided steps carry the keyword
    monkeypatch.delenv("SEVA_GUIDANCE_INTERVAL")
    _, b, cl = run(guidance_interval=INTERVAL)
    assert cl == [(8, [] if g else ["guided"]) for g in GUIDED]


def test_subclass_that_drives_the_steps_itself_gets_guided_steps(cpu_sampler):
    S = cpu_sampler

    class Tracked(S.EulerEDMSampler):  # the reference's GradioTrackedSampler pattern
        def __call__(self, denoiser, x, scale, cond, uc=None, num_steps=None, verbose=True, **guider_kwargs):
            x, s_in, sigmas, num_sigmas, cond, uc = self.prepare_sampling_loop(x, cond, cond if uc is None else uc, num_steps)
            for i in self.get_sigma_gen(num_sigmas, verbose=verbose):
                x = self.sampler_step(s_in * sigmas[i], s_in * sigmas[i + 1], denoiser, x, scale, cond, uc, 0.0, **guider_kwargs)
            return x

    net = Net()
    _trajectory(_sampler(S, "euler", cls=Tracked, guidance_interval=INTERVAL), net)
    assert net.batches == [2 * N] * STEPS


def _unguided_loop(S, solver, net, seed=1):
    """The trajectory of an interval that guides nothing, written out: the denoiser on the conditional inputs, then
    `ops.euler_step`, or `ops.cfg_multistep(scale=None)` under dpmpp2m."""
    import seva.ops as ops
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(100 + seed))
    cond, _ = _cond()
    sigmas = S.DDPMDiscretization()(STEPS)
    x = x * torch.sqrt(1.0 + sigmas[0] ** 2.0)
    s_in = x.new_ones([N])
    hist, prev = torch.zeros_like(x), torch.zeros(N)
    for i in range(STEPS):
        sigma, nxt = s_in * sigmas[i], s_in * sigmas[i + 1]
        out = torch.empty_like(x)
        if solver == "euler":
            eps = torch.randn(x.shape, generator=g)
            sigma_hat = sigma * (0.0 + 1.0) + 1e-6
            x_in = torch.empty_like(x)
            ops.add_noise(x, eps, (sigma_hat**2 - sigma**2) ** 0.5 * 1.0, x_in)
            ops.euler_step(x_in, net(x_in, sigma_hat, cond), sigma_hat, nxt - sigma_hat, out)
        else:
            a, b, c = S.EulerEDMSampler.multistep_coefficients(sigma, nxt, prev)
            ops.cfg_multistep(x, net(x, sigma, cond), None, hist, a, b, c, out, hist)
            prev = sigma
        x = out
    return x


@pytest.mark.parametrize("solver", ["euler", "dpmpp2m"])
def test_an_interval_that_guides_nothing_is_the_conditional_loop(cpu_sampler, solver):
    S = cpu_sampler
    net, calls = Net(), []
    got = _trajectory(_sampler(S, solver, guider=_guider(S, calls), guidance_interval=(100.0, 200.0)), net)
    want_net = Net()
    want = _unguided_loop(S, solver, want_net)
    assert torch.equal(got, want) and net.batches == want_net.batches == [N] * STEPS and not calls
    # rescale has nothing to act on where no step is guided
    assert torch.equal(_trajectory(_sampler(S, solver, guidance_interval=(100.0, 200.0), guidance_rescale=0.7), Net()), want)


def test_unguided_step_leaves_the_callers_cond_alone(cpu_sampler):
    """`DiscreteDenoiser` pops "replace" from the dictionary it is handed; the unguided step hands it a copy."""
    S = cpu_sampler
    seen = []

    def popping(xx, ss, cc):
        seen.append("replace" in cc)
        cc.pop("replace", None)
        return 0.5 * xx

    cond = {"vector": torch.ones(N, 1), "replace": torch.zeros(N, 1)}
    sm = _sampler(S, "euler", steps=4, guidance_interval=(100.0, 200.0))
    sm.noise_fn = torch.zeros_like
    sm(popping, torch.ones(SHAPE), SCALE, cond, dict(cond), verbose=False)
    assert seen == [True] * 4 and "replace" in cond


# ------------------------------------------------------------------------------------------------ with cache_interval
@pytest.mark.parametrize("solver", ["euler", "dpmpp2m"])
def test_step_kinds_with_cache_interval(cpu_sampler, solver):
    S = cpu_sampler
    net = Net()
    _trajectory(_sampler(S, solver, guidance_interval=INTERVAL, cache_interval=3, cache_levels=2), net)
    kinds = " ".join("S" if L else "F" for L in net.levels)
    assert kinds == "F S S F S S F S F F"  # step 8: forced full by the boundary (step 3 is full by i % 3 anyway); step 9: the last
    assert net.batches == [2 * N if g else N for g in GUIDED] and set(net.levels) == {0, 2}
    # a boundary that does not fall on a multiple of the interval: (5, 40) guides steps 2..6
    net = Net()
    _trajectory(_sampler(S, solver, guidance_interval=(5.0, 40.0), cache_interval=3), net)
    assert [b == 2 * N for b in net.batches] == [False, False, True, True, True, True, True, False, False, False]
    assert " ".join("S" if L else "F" for L in net.levels) == "F S F F S S F F S F"
    # every shallow call has a full call of the same batch directly behind its run of shallow calls
    last_full = None
    for b, L in zip(net.batches, net.levels):
        if L == 0:
            last_full = b
        assert b == last_full


# ------------------------------------------------------------------------------------------------ whole-step graphs
@pytest.mark.parametrize("solver", ["euler", "dpmpp2m"])
def test_step_kinds_take_distinct_graph_entries(cpu_sampler, monkeypatch, solver):
    from seva import _stepgraph
    S = cpu_sampler
    monkeypatch.setattr(_stepgraph, "StepGraph", FakeStepGraph)
    monkeypatch.setattr(S.EulerEDMSampler, "_whole_step_graph_eligible", lambda self, x: not self._step_graphs.disabled)
    kw = dict(guidance_interval=INTERVAL, guidance_rescale=0.7, cache_interval=3, cache_levels=2)
    ref = _trajectory(_sampler(S, solver, **kw), Net())
    sm = _sampler(S, solver, **kw)
    sm._step_graphs.disabled = False
    net = Net()
    got = _trajectory(sm, net)
    cache = sm._step_graphs
    assert torch.equal(got, ref) and not cache.disabled
    # F S S F S S F S F F over unguided 0..2, guided 3..7, unguided 8..9
    U0, U2 = (0, "unguided"), (2, "unguided")
    assert set(cache.entries) == {0, 2, U0, U2}
    replays = {k: (e.graph.replays if e.graph is not None else None) for k, e in cache.entries.items()}
    # unguided full 0 8 9: warm-up, capture, replay; unguided shallow 1 2: warm-up, capture; guided full 3 6; guided shallow 4 5 7
    assert replays == {U0: 2, U2: 1, 0: 1, 2: 2} and cache.captures == 4
    assert len({id(e.graph) for e in cache.entries.values()}) == 4
    assert "unguided" in cache.entries[U0].key and "unguided" not in cache.entries[0].key
    assert cache.entries[0].key[-2:] == ("rescale", 0.7) and cache.entries[2].key[-2:] == ("rescale", 0.7)  # phi is part of the key
    # another phi through the same sampler: the guided entries are captured again, the unguided ones are not
    sm.guidance_rescale = 0.5
    ref2 = _trajectory(_sampler(S, solver, **dict(kw, guidance_rescale=0.5)), Net())
    assert torch.equal(_trajectory(sm, net), ref2) and not torch.equal(ref2, ref)  # (the same denoiser object: it is part of every key)
    assert cache.captures == 6 and cache.entries[U0].graph.replays == 2 + 3 and cache.entries[0].key[-1] == 0.5
    # with the feature off the kinds and the keys are the ones of before
    off = _sampler(S, solver, cache_interval=3, cache_levels=2)
    off._step_graphs.disabled = False
    _trajectory(off, Net())
    assert set(off._step_graphs.entries) == {0, 2}
    assert not any(v in ("unguided", "rescale") for e in off._step_graphs.entries.values() for v in e.key if isinstance(v, str))


# ------------------------------------------------------------------------------------------------ rescale
def _moderate(n, shape, seed):
    """[uncond ; cond] with |mean| <= std per frame (mean 0.5, std 1 and 1.5)"""
    g = torch.Generator().manual_seed(seed)
    u = 0.5 + torch.randn((n,) + shape, generator=g)
    c = -0.5 + 1.5 * torch.randn((n,) + shape, generator=g)
    return torch.cat([u, c])


def test_emulated_rescale_restores_the_conditional_std():
    n, shape = 5, (4, 9, 7)
    den2 = _moderate(n, shape, 3)
    scale = torch.tensor([0.0, 1.0, 2.0, 4.5, 3.0])
    g = torch.empty((n,) + shape)
    import fake_ops
    fake_ops.cfg_combine(den2, scale, g)
    cond = den2.chunk(2)[1]
    std = lambda t: t.reshape(n, -1).double().std(1)  # noqa: E731
    assert float((cond.reshape(n, -1).mean(1).abs() / std(cond)).max()) <= 1.0
    out, m = torch.empty_like(g), torch.empty(n)
    fake_guidance_ops.cfg_rescale(den2, scale, 1.0, out, m)
    rel = ((std(out) - std(cond)).abs() / std(cond)).max()
    print(f"phi = 1: per-frame std of D vs the cond half, max relative difference {float(rel):.2e}; m = {m.tolist()}")
    assert float(rel) <= 1e-6
    assert m[1] == 1.0 and torch.equal(out[1], g[1])  # scale 1: g IS the cond half
    assert m[3] < 1.0 and m[0] > 1.0  # cfg 4.5 inflates the std, scale 0 (the narrower uncond half) deflates it
    # phi blends the multiplier linearly, phi = 0 is cfg_combine
    out7, m7 = torch.empty_like(g), torch.empty(n)
    fake_guidance_ops.cfg_rescale(den2, scale, 0.7, out7, m7)
    p = float(torch.tensor(0.7, dtype=torch.float32))
    assert torch.allclose(m7.double(), p * m.double() + (1 - p), rtol=2e-7, atol=0)
    fake_guidance_ops.cfg_rescale(den2, scale, 0.0, out7, m7)
    assert torch.equal(out7, g) and torch.equal(m7, torch.ones(n))
    # the selects: a constant frame and a one-element frame give exactly 1
    flat = torch.cat([torch.full((2, 6), 0.75), torch.full((2, 6), -1.5)])
    o, mm = torch.empty(2, 6), torch.empty(2)
    fake_guidance_ops.cfg_rescale(flat, torch.tensor([2.0, 4.5]), 1.0, o, mm)
    assert torch.equal(mm, torch.ones(2)) and torch.equal(o[0], torch.full((6,), 0.75 + 2.0 * (-1.5 - 0.75)))
    one = torch.tensor([[0.3], [-0.2]])
    fake_guidance_ops.cfg_rescale(one, torch.tensor([3.0]), 1.0, o[:1, :1], mm[:1])
    assert mm[0] == 1.0
    with pytest.raises(ValueError):
        fake_guidance_ops.cfg_rescale(den2, scale, 1.5, out, m)


@pytest.mark.parametrize("solver", ["euler", "dpmpp2m"])
def test_rescaled_steps_are_the_loop_written_out(cpu_sampler, monkeypatch, solver):
    """Guided steps with phi > 0: D = `ops.cfg_rescale(den2, frame_scale, phi)`, then `ops.euler_step` or
    `ops.cfg_multistep(scale=None)` on D; with phi == 0 the old fused path, and `ops.cfg_rescale` is never called."""
    import seva.ops as ops
    S = cpu_sampler
    log = []
    for name in ("cfg_rescale", "cfg_euler", "euler_step", "cfg_multistep"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _r=real, **k: (log.append((_n, a)), _r(*a, **k))[1])
    phi = 0.7
    got = _trajectory(_sampler(S, solver, guidance_interval=INTERVAL, guidance_rescale=phi), Net())
    names = [n for n, _ in log]
    update = "euler_step" if solver == "euler" else "cfg_multistep"
    assert names == [update] * 3 + ["cfg_rescale", update] * 5 + [update] * 2
    for (n, a), (n2, a2) in zip(log, log[1:]):
        if n == "cfg_rescale":
            assert a[0].shape[0] == 2 * N and torch.equal(a[1], torch.full((N,), SCALE)) and a[2] == phi
            assert a2[1] is a[3] and (solver == "euler" or a2[2] is None)  # the update reads the D that cfg_rescale wrote
    # the same trajectory as a loop over the ops
    g = torch.Generator().manual_seed(1)
    x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(101))
    cond, uc = _cond()
    net, guider = Net(), S.VanillaCFG()
    sigmas = S.DDPMDiscretization()(STEPS)
    x = x * torch.sqrt(1.0 + sigmas[0] ** 2.0)
    s_in = x.new_ones([N])
    hist, prev = torch.zeros_like(x), torch.zeros(N)
    fs = torch.full((N,), SCALE)
    for i in range(STEPS):
        sigma, nxt = s_in * sigmas[i], s_in * sigmas[i + 1]
        out = torch.empty_like(x)
        if solver == "euler":
            sigma_in = sigma * (0.0 + 1.0) + 1e-6
            x_in = torch.empty_like(x)
            fake_add = (sigma_in**2 - sigma**2) ** 0.5 * 1.0
            ops.add_noise(x, torch.randn(x.shape, generator=g), fake_add, x_in)
        else:
            sigma_in, x_in = sigma, x
        if GUIDED[i]:
            D = torch.empty_like(x)
            fake_guidance_ops.cfg_rescale(net(*guider.prepare_inputs(x_in, sigma_in, cond, uc)), fs, phi, D)
        else:
            D = net(x_in, sigma_in, cond)
        if solver == "euler":
            ops.euler_step(x_in, D, sigma_in, nxt - sigma_in, out)
        else:
            a, b, c = S.EulerEDMSampler.multistep_coefficients(sigma, nxt, prev)
            _fake_cfg_multistep(x, D, None, hist, a, b, c, out, hist)
            prev = sigma
        x = out
    assert torch.equal(got, x)
    # phi == 0: the fused path of before
    del log[:]
    _trajectory(_sampler(S, solver, guidance_interval=INTERVAL, guidance_rescale=0.0), Net())
    fused = "cfg_euler" if solver == "euler" else "cfg_multistep"
    assert [n for n, _ in log] == [update] * 3 + [fused] * 5 + [update] * 2
    assert all(a[2] is not None for n, a in log[3:8])  # the guided steps hand the kernel the scale vector
    del log[:]
    off = _trajectory(_sampler(S, solver), Net())
    assert [n for n, _ in log] == [fused] * STEPS
    # and rescale alone (no interval) acts on every step and changes the result
    del log[:]
    resc = _trajectory(_sampler(S, solver, guidance_rescale=phi), Net())
    assert [n for n, _ in log] == ["cfg_rescale", update] * STEPS and not torch.equal(resc, off)


def test_rescale_needs_a_guider_that_states_its_frame_scale(cpu_sampler):
    S = cpu_sampler

    class PlainGuider:
        def prepare_inputs(self, x, s, c, uc):
            return S.VanillaCFG().prepare_inputs(x, s, c, uc)

        def __call__(self, x, sigma, scale):
            u, c = x.chunk(2)
            return u + scale * (c - u)

    for solver in ("euler", "dpmpp2m"):
        with pytest.raises(ValueError, match="frame_scale"):
            _trajectory(_sampler(S, solver, guider=PlainGuider(), guidance_rescale=0.5), Net())
        # without rescale such a guider works, inside and outside an interval
        out = _trajectory(_sampler(S, solver, guider=PlainGuider(), guidance_interval=INTERVAL), Net())
        assert torch.equal(out, _trajectory(_sampler(S, solver, guidance_interval=INTERVAL), Net()))


# ------------------------------------------------------------------------------------------------ two ranks under cfg_split
def _split_worker(rank, port, q, solver, kw):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2")
    for name in ENV:
        os.environ.pop(name, None)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=2)
    _install()
    from seva import sampling as S
    net, gathers = Net(), []
    real = dist.all_gather_into_tensor

    def counting(out, inp, group=None):
        gathers.append(len(net.batches) - 1)  # the step whose network call has just returned
        return real(out, inp, group=group)

    dist.all_gather_into_tensor = counting
    sm = _sampler(S, solver, **kw)
    sm.cfg_split = (dist.group.WORLD, rank)
    out = _trajectory(sm, net)
    q.put((rank, out.numpy(), gathers, net.batches, net.levels))
    dist.destroy_process_group()


@pytest.mark.parametrize("solver", ["euler", "dpmpp2m"])
def test_two_ranks_under_cfg_split(cpu_sampler, solver):
    from conftest import PKG
    S = cpu_sampler
    here = os.path.dirname(os.path.abspath(__file__))
    os.environ["PYTHONPATH"] = os.pathsep.join([PKG, here, os.environ.get("PYTHONPATH", "")])
    kw = dict(guidance_interval=INTERVAL, guidance_rescale=0.7, cache_interval=3)
    ref_net = Net()
    ref = _trajectory(_sampler(S, solver, **kw), ref_net)
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_split_worker, args=(r, port, q, solver, kw)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in range(2)), key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank, out, gathers, batches, levels in res:
        assert torch.equal(torch.from_numpy(out), ref), rank  # both ranks hold the single process's bits
        assert gathers == [3, 4, 5, 6, 7]                      # one collective per guided step, none on the others
        assert batches == [N] * STEPS and levels == ref_net.levels  # a half batch or the conditional batch: n rows either way


# ------------------------------------------------------------------------------------------------ drivers
def test_drivers_hand_the_values_to_every_window(cpu_sampler, monkeypatch):
    from seva import pipeline
    seen = []
    c2ws, Ks, lat, tok = _scene(43)

    def run(fn=pipeline.run_trajectory, **kw):
        del seen[:]
        return fn(_fake_net, lat, c2ws, Ks, [0], clip_token=tok, T=21, num_steps=3, seed=23, device="cpu",
                  sampler_hook=lambda sm: seen.append((sm.guidance_interval, sm.guidance_rescale)), **kw)

    res = run()
    plan, base = res["plan"], res["latents"]
    n1, n2 = len(plan.pass1), len(plan.pass2)
    assert n1 >= 1 and n2 >= 1 and seen == [(None, 0.0)] * (n1 + n2)
    out = run(guidance_interval=(0.3, 5), guidance_rescale=0.7)
    assert seen == [((0.3, 5.0), 0.7)] * (n1 + n2) and torch.isfinite(out["latents"]).all() and not torch.equal(out["latents"], base)
    run(guidance_interval=((0.5, 3), None), guidance_rescale=(0.0, 0.5))
    assert seen == [((0.5, 3.0), 0.0)] * n1 + [(None, 0.5)] * n2
    run(guidance_interval=(None, (1, INF)), guidance_rescale=1)
    assert seen == [(None, 1.0)] * n1 + [((1.0, INF), 1.0)] * n2
    run(guidance_interval=("0.3,5", (0.5, 3)))
    assert seen == [((0.3, 5.0), 0.0)] * n1 + [((0.5, 3.0), 0.0)] * n2
    run(guidance_interval="0.3,5")
    assert seen == [((0.3, 5.0), 0.0)] * (n1 + n2)
    run(pipeline.run_views, guidance_interval=(0.5, 3), guidance_rescale=0.25)
    assert seen and set(seen) == {((0.5, 3.0), 0.25)}
    assert torch.equal(run(guidance_interval=(0, INF), guidance_rescale=0)["latents"], base)
    monkeypatch.setenv("SEVA_GUIDANCE_INTERVAL", "0.5,3")
    monkeypatch.setenv("SEVA_GUIDANCE_RESCALE", "0.7")
    run()
    assert seen == [((0.5, 3.0), 0.7)] * (n1 + n2)
    run(guidance_interval=((0.3, 5), None), guidance_rescale=(None, 0))  # None: that pass reads the variables
    assert seen == [((0.3, 5.0), 0.7)] * n1 + [((0.5, 3.0), 0.0)] * n2
    # one window, directly
    win = plan.pass1[0]
    noise = torch.randn((len(win.slot_frame), 4, 8, 8), generator=torch.Generator().manual_seed(0))
    pipeline.run_window(win, {0: lat[0]}, _fake_net, c2ws, Ks, hw=(8, 8), num_steps=3, cfg=2.0, cfg_min=1.2, guider=1, camera_scale=2.0,
                        noise=noise, step_seed=1, clip_token=tok, device="cpu", guidance_interval=(1, 2), guidance_rescale=0.1,
                        sampler_hook=lambda sm: seen.append(("window", sm.guidance_interval, sm.guidance_rescale)))
    assert seen[-1] == ("window", (1.0, 2.0), 0.1)
    with pytest.raises(ValueError):
        run(guidance_interval=(5, 0.3))


def test_run_scene_accepts_the_arguments():
    import inspect
    from seva import pipeline
    for fn in (pipeline.run_window, pipeline.run_trajectory):
        assert {"guidance_interval", "guidance_rescale"} <= set(inspect.signature(fn).parameters)
    for fn in (pipeline.run_views, pipeline.run_scene):  # hand every sampler option on to run_trajectory
        assert "run_trajectory_kwargs" in inspect.signature(fn).parameters and "guidance_rescale" in fn.__doc__
