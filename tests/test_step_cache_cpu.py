"""Opt-in reuse of deep UNet features across sampler steps, host side: `SevaEngine.forward(shallow_levels=L)` with tests/fake_ops.py
as the kernels (bit equality with the full call on the same inputs, the CPU oracle on other inputs, the guard), the sampler's
schedule and defaults (`EulerEDMSampler(cache_interval=, cache_levels=)`, SEVA_CACHE_INTERVAL / SEVA_CACHE_LEVELS), the drivers,
and the whole-step graph entries of the two step kinds (the stand-in graph of tests/test_stepgraph_cpu.py)."""
import pytest
import torch
import torch.nn.functional as F

import fake_ops
from conftest import load_golden, rel_l2
from test_engine_host_logic import _cpu_engine, _shapes
from test_pipeline_cpu import _fake_net, _patch_cpu, _scene
from test_solver_dpmpp2m_cpu import SCALE, SHAPE, _fake_cfg_multistep, _rows
from test_stepgraph_cpu import FakeStepGraph

JOINT = ("middle_ds8", "output_ds4", "output_ds2")
BLOCKS = {1: 2, 2: 5, 3: 8}  # input blocks after the stem that a shallow call of depth L runs (this architecture)


class CountingOps:
    """tests/fake_ops.py behind a launch counter: every call is booked under the scope that the engine last marked."""

    def __init__(self):
        self.scope, self.calls = None, []

    def mark(self, scope):
        self.scope = scope

    def __getattr__(self, name):
        v = getattr(fake_ops, name)
        if not callable(v):
            return v

        def counted(*a, **k):
            self.calls.append((self.scope, name))
            return v(*a, **k)

        return counted


@pytest.fixture()
def counting(monkeypatch):
    from seva import _engine
    ops = CountingOps()
    monkeypatch.setattr(_engine, "ops", ops)
    monkeypatch.setattr(_engine, "audit_mark", ops.mark)
    monkeypatch.setattr(_engine, "require_cuda", lambda *a: None)
    return ops


def _inputs(T, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    n = 2 * T
    return (torch.randn(n, 11, h, w, generator=g), None, torch.randint(0, 1000, (n,), generator=g),
            torch.randn(n, 1, 1024, generator=g), torch.randn(n, 6, h, w, generator=g), T)


def _golden_inputs():
    g = load_golden("g3_tiny_forward")
    return g["x"], g["concat"], g["t"], g["crossattn"], g["dense_vector"], int(g["T"])


def _entry_name(eng, L):
    """arena name of the tensor that enters the first output block a shallow call of depth L runs"""
    first = len(eng.layout.output_blocks) - (eng.shallow_input_blocks(L) + 1)
    return "out:" + eng.layout.output_blocks[first - 1][-1].prefix


def _allowed_scopes(eng, L):
    m = eng.shallow_input_blocks(L)
    blocks = eng.layout.input_blocks[:1 + m] + eng.layout.output_blocks[len(eng.layout.output_blocks) - (m + 1):]
    return ("time_embed", "out") + tuple(spec.prefix for blk in blocks for spec in blk)


@pytest.mark.parametrize("case", ["g3_tiny_forward", "T3_8x24", "T2_32x32_stats2"])
def test_shallow_call_on_the_same_inputs_is_the_full_call(counting, case):
    eng, _ = _cpu_engine()
    assert [eng.shallow_input_blocks(L) for L in (1, 2, 3)] == [BLOCKS[L] for L in (1, 2, 3)]
    if case == "g3_tiny_forward":
        args = _golden_inputs()
    elif case == "T3_8x24":
        args = _inputs(3, 8, 24, 5)
    else:
        args = _inputs(2, 32, 32, 7)
        eng.gn_fused_stats = 2
    full = eng.forward(*args).clone()
    n_full = len(counting.calls)
    travelled = 0
    for L in (1, 2, 3):
        name = _entry_name(eng, L)
        (buf,) = [t for k, t in eng.arena.bufs.items() if k[0] == name]
        entry = eng._shallow_entries[eng._last_full][L]
        stats = entry.stats
        assert entry.t is buf
        travelled += stats is not None
        before, st_before = buf.clone(), None if stats is None else stats.clone()
        del counting.calls[:]
        out = eng.forward(*args, shallow_levels=L)
        assert torch.equal(out, full), (case, L)
        assert torch.equal(buf, before) and (stats is None or torch.equal(stats, st_before))
        # nothing launched outside the blocks a shallow call runs, and far fewer launches than the full call
        allowed = _allowed_scopes(eng, L)
        stray = sorted({s for s, _ in counting.calls if not any(s == a or s.startswith(a + ".") for a in allowed)})
        assert not stray, (L, stray)
        assert not any(s.startswith("middle_block") for s, _ in counting.calls) and 0 < len(counting.calls) < n_full
        print(f"{case} L={L}: {len(counting.calls)} of {n_full} launches; statistics travel: {stats is not None}")
    if case == "T2_32x32_stats2":
        assert travelled >= 1  # a producer's statistics buffer did travel with a reused tensor
    # a shallow call is no full call: the guard still names the full call's signature, and a full call can follow
    assert torch.equal(eng.forward(*args), full)


def _oracle_shallow(sd, x, t, y, dense, T, L, trace_full):
    """The CPU oracle's network run shallow: input blocks above the L-th Downsample and the matching output blocks at (x, t, y,
    dense), fed at the entry point from `trace_full`, the trace of a full oracle run at OTHER inputs."""
    from oracle import seva_ref as O
    emb = O.timestep_embedding(t, sd["time_embed.0.weight"].shape[1])
    emb = O.linear(sd, "time_embed.2", F.silu(O.linear(sd, "time_embed.0", emb)))
    downs = [i for i in O._sublayers(sd, "input_blocks") if f"input_blocks.{i}.0.op.weight" in sd]
    m = downs[L - 1] - 1
    hs, h, ds = [], x, 1
    for i in range(m + 1):
        h, dch = O._run_sequential(sd, f"input_blocks.{i}", h, emb, y, dense, T, f"input_ds{ds}", JOINT)
        ds *= 2 if dch > 0 else 1
        hs.append(h)
    nout = len(O._sublayers(sd, "output_blocks"))
    first = nout - (m + 1)
    h = trace_full[f"output_blocks.{first - 1}.{O._sublayers(sd, f'output_blocks.{first - 1}')[-1]}"]
    for i in range(first, nout):
        h, dch = O._run_sequential(sd, f"output_blocks.{i}", torch.cat([h, hs.pop()], 1), emb, y, dense, T, f"output_ds{ds}", JOINT)
        ds //= 2 if dch < 0 else 1
    return O.conv2d(sd, "out.2", F.silu(O.group_norm(sd, "out.0", h, 1e-5)))


@pytest.mark.parametrize("L", [1, 2, 3])
def test_shallow_call_on_other_inputs_vs_the_oracle(counting, L):
    """Full at (x1, t1, c1), shallow at (x2, t2, c2) against the oracle composed the same way, held to the bound of
    `test_engine_orchestration_vs_oracle` for the emulated kernels; and the result is NOT the full call's at (x2, t2, c2)."""
    from oracle import seva_ref as O
    eng, sd = _cpu_engine()
    x1, c1, t1, y1, d1, T = _golden_inputs()
    g = torch.Generator().manual_seed(91)
    x2, c2, y2, d2 = (torch.randn(v.shape, generator=g) for v in (x1, c1, y1, d1))
    t2 = torch.randint(0, 1000, t1.shape, generator=g)
    full2 = eng.forward(x2, c2, t2, y2, d2, T).clone()
    trace = {}
    O.seva_forward(sd, torch.cat([x1, c1], 1), t1, y1, d1, T, trace=trace)
    eng.forward(x1, c1, t1, y1, d1, T)
    got = eng.forward(x2, c2, t2, y2, d2, T, shallow_levels=L)
    ref = _oracle_shallow(sd, torch.cat([x2, c2], 1), t2, y2, d2, T, L, trace)
    err, full_err = rel_l2(got, ref), rel_l2(full2, O.seva_forward(sd, torch.cat([x2, c2], 1), t2, y2, d2, T))
    away = rel_l2(got, full2)
    print(f"L={L}: shallow vs composed oracle {err:.2e} (the full call's own error at these inputs {full_err:.2e}); "
          f"shallow vs full call at the same inputs {away:.2e}")
    assert err < 2e-3
    assert away > 2e-3  # a path that ignores the flag cannot pass both


def test_guard(counting, monkeypatch):
    from seva import _engine
    from seva import synthetic as synth
    from seva._native import SevaNativeError
    from seva.model import Seva, SevaParams
    eng, _ = _cpu_engine()
    a, b, c = _inputs(2, 8, 8, 1), _inputs(3, 8, 8, 2), _inputs(2, 8, 16, 3)
    with pytest.raises(SevaNativeError, match="no full call"):
        eng.forward(*a, shallow_levels=1)
    for bad in (4, -1):
        with pytest.raises(ValueError):
            eng.forward(*a, shallow_levels=bad)
    full = eng.forward(*a).clone()
    assert torch.equal(eng.forward(*a, shallow_levels=2), full)
    eng.forward(*b)  # another T in between
    with pytest.raises(SevaNativeError, match="num_frames 3 -> 2"):
        eng.forward(*a, shallow_levels=2)
    eng.forward(*a)
    eng.forward(*c)  # another size in between
    with pytest.raises(SevaNativeError, match=r"x \(4, 11, 8, 16\) -> \(4, 11, 8, 8\)"):
        eng.forward(*a, shallow_levels=1)
    # a failed guard is no full call, and no fall-back to one: the next shallow call of the size that DID run last passes
    launches = len(counting.calls)
    with pytest.raises(SevaNativeError):
        eng.forward(*a, shallow_levels=1)
    assert len(counting.calls) == launches
    assert torch.equal(eng.forward(*c, shallow_levels=1), eng.forward(*c))
    # a full call that fails half way leaves nothing to reuse
    with monkeypatch.context() as mp:
        mp.setattr(eng, "_transformer", lambda *a, **k: (_ for _ in ()).throw(RuntimeError("boom")))
        with pytest.raises(RuntimeError, match="boom"):
            eng.forward(*c)
    with pytest.raises(SevaNativeError, match="no full call"):
        eng.forward(*c, shallow_levels=1)
    # a rebuilt engine (set_precision) starts without a full call
    with torch.device("meta"):
        net = Seva(SevaParams(model_channels=64))
    net.load_state_dict(synth.synth_state_dict(_shapes("tiny")), strict=True, assign=True)
    monkeypatch.setattr(_engine.SevaEngine, "_resolve_device", staticmethod(lambda m: torch.device("cpu")))
    first = net.engine()
    full = first.forward(*a).clone()
    assert torch.equal(first.forward(*a, shallow_levels=1), full)
    rebuilt = net.set_precision("f16").engine()
    assert rebuilt is not first
    with pytest.raises(SevaNativeError, match="no full call"):
        rebuilt.forward(*a, shallow_levels=1)


def test_request_travels_through_the_context(counting, monkeypatch):
    """`_native.shallow_network(L)` is read in `SevaEngine.__call__`, nests, and ends with its block."""
    from seva import _native
    eng, _ = _cpu_engine()
    eng.use_graph = False
    seen = []
    real = eng.forward
    monkeypatch.setattr(eng, "forward", lambda *a, **k: (seen.append(k.get("shallow_levels")), real(*a, **k))[1])
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    a = _inputs(2, 8, 8, 1)
    full = eng(*a).clone()
    with _native.shallow_network(2):
        assert _native.network_shallow_levels() == 2 and torch.equal(eng(*a), full)
        with _native.shallow_network(0):
            eng(*a)
        with _native.shallow_network(1):
            eng(*a)
        assert _native.network_shallow_levels() == 2
    eng(*a)
    assert seen == [0, 2, 0, 1, 0] and _native.network_shallow_levels() == 0
    with pytest.raises(RuntimeError, match="boom"):
        with _native.shallow_network(3):
            raise RuntimeError("boom")
    assert _native.network_shallow_levels() == 0


# ------------------------------------------------------------------------------------------------ sampler
@pytest.fixture
def cpu_sampler(monkeypatch):
    import seva.ops as ops
    from seva import sampling as S
    for name in ("SEVA_SOLVER", "SEVA_CACHE_INTERVAL", "SEVA_CACHE_LEVELS"):
        monkeypatch.delenv(name, raising=False)
    _patch_cpu(monkeypatch)
    monkeypatch.setattr(ops, "cfg_multistep", _fake_cfg_multistep, raising=False)
    return S


class Recorder:
    """A stand-in network behind the sampler's opaque denoiser: records the depth requested for each call.  Shallow calls return
    another function of the inputs, so a schedule that differs shows in the result too."""

    def __init__(self):
        self.levels = []

    def __call__(self, xx, ss, cc):
        from seva import _native
        L = _native.network_shallow_levels()
        self.levels.append(L)
        k = _rows(1.0 / (1.0 + ss * ss), xx)
        return (0.1 + 0.05 * L) * (1 - k) + xx * k


def _sampler(S, solver, steps, churn=0.0, **kw):
    sm = S.EulerEDMSampler(S.DDPMDiscretization(), S.VanillaCFG(), num_steps=steps, verbose=False, device="cpu", solver=solver,
                           s_churn=churn, **kw)
    sm._step_graphs.disabled = True
    return sm


def _trajectory(sm, net, seed=1):
    g = torch.Generator().manual_seed(seed)
    sm.noise_fn = lambda x: torch.randn(x.shape, generator=g)
    x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(100 + seed))
    return sm(net, x, SCALE, {}, {}, verbose=False)


def _expected(steps, N, L):
    return [0 if i % N == 0 or i == steps - 1 else L for i in range(steps)]


@pytest.mark.parametrize("solver,churn", [("euler", 0.0), ("euler", 0.5), ("dpmpp2m", 0.0)])
@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("L", [1, 2])
def test_schedule(cpu_sampler, solver, churn, N, L):
    S = cpu_sampler
    steps = 7
    net = Recorder()
    out = _trajectory(_sampler(S, solver, steps, churn, cache_interval=N, cache_levels=L), net)
    assert net.levels == _expected(steps, N, L), net.levels
    assert {2: [0, L, 0, L, 0, L, 0], 3: [0, L, L, 0, L, L, 0]}[N] == net.levels
    plain = Recorder()
    assert not torch.equal(out, _trajectory(_sampler(S, solver, steps, churn), plain)) and plain.levels == [0] * steps


def test_schedule_ends_on_a_full_step_and_short_trajectories(cpu_sampler):
    S = cpu_sampler
    for steps, N, want in ((6, 2, [0, 1, 0, 1, 0, 0]), (6, 5, [0, 1, 1, 1, 1, 0]), (2, 2, [0, 0]), (1, 3, [0]), (3, 7, [0, 1, 0])):
        net = Recorder()
        _trajectory(_sampler(S, "euler", steps, cache_interval=N), net)
        assert net.levels == want == _expected(steps, N, 1), (steps, N, net.levels)


@pytest.mark.parametrize("solver,churn", [("euler", 0.0), ("euler", 0.5), ("dpmpp2m", 0.0)])
def test_mode_off_is_the_sampler_without_the_arguments(cpu_sampler, monkeypatch, solver, churn):
    S = cpu_sampler
    steps = 5
    calls = []

    class Spy(S.EulerEDMSampler):  # the calls `__call__` makes, keyword for keyword
        def sampler_step(self, *a, **k):
            calls.append((len(a), sorted(k)))
            return super().sampler_step(*a, **k)

    def run(**kw):
        del calls[:]
        net = Recorder()
        sm = Spy(S.DDPMDiscretization(), S.VanillaCFG(), num_steps=steps, verbose=False, device="cpu", solver=solver, s_churn=churn, **kw)
        sm._step_graphs.disabled = True
        return _trajectory(sm, net), net.levels, list(calls), sm

    ref, levels, ref_calls, sm = run()
    assert (sm.cache_interval, sm.cache_levels) == (0, 1) and levels == [0] * steps and ref_calls == [(8, [])] * steps
    for kw in (dict(cache_interval=0), dict(cache_interval=1), dict(cache_interval=None, cache_levels=3), dict(cache_interval=1, cache_levels=2)):
        out, lv, cl, sm = run(**kw)
        assert torch.equal(out, ref) and lv == levels and cl == ref_calls and sm.cache_interval == 0, kw
    for env in ("0", "1", ""):
        monkeypatch.setenv("SEVA_CACHE_INTERVAL", env)
        out, lv, cl, sm = run()
        assert torch.equal(out, ref) and lv == levels and cl == ref_calls and sm.cache_interval == 0, env
    # and with the mode on, only the shallow steps carry the keyword
    monkeypatch.delenv("SEVA_CACHE_INTERVAL")
    _, lv, cl, _ = run(cache_interval=2)
    assert cl == [(8, ["shallow"] if v else []) for v in lv] and lv == [0, 1, 0, 1, 0]


def test_subclass_that_drives_the_steps_itself_gets_full_steps(cpu_sampler):
    S = cpu_sampler

    class Tracked(S.EulerEDMSampler):  # the reference's GradioTrackedSampler pattern
        def __call__(self, denoiser, x, scale, cond, uc=None, num_steps=None, verbose=True, **guider_kwargs):
            x, s_in, sigmas, num_sigmas, cond, uc = self.prepare_sampling_loop(x, cond, cond if uc is None else uc, num_steps)
            for i in self.get_sigma_gen(num_sigmas, verbose=verbose):
                x = self.sampler_step(s_in * sigmas[i], s_in * sigmas[i + 1], denoiser, x, scale, cond, uc, 0.0, **guider_kwargs)
            return x

    net = Recorder()
    sm = Tracked(S.DDPMDiscretization(), S.VanillaCFG(), num_steps=5, verbose=False, device="cpu", cache_interval=2)
    sm._step_graphs.disabled = True
    _trajectory(sm, net)
    assert sm.cache_interval == 2 and net.levels == [0] * 5


def test_arguments_and_environment(cpu_sampler, monkeypatch):
    S = cpu_sampler
    mk = lambda **kw: S.EulerEDMSampler(S.DDPMDiscretization(), S.VanillaCFG(), num_steps=3, device="cpu", **kw)  # noqa: E731
    got = lambda sm: (sm.cache_interval, sm.cache_levels)  # noqa: E731
    assert got(mk()) == (0, 1) and got(mk(cache_interval=4)) == (4, 1) and got(mk(cache_interval=2, cache_levels=3)) == (2, 3)
    monkeypatch.setenv("SEVA_CACHE_INTERVAL", "3")
    assert got(mk()) == (3, 1) and got(mk(cache_levels=2)) == (3, 2)
    monkeypatch.setenv("SEVA_CACHE_LEVELS", "2")
    assert got(mk()) == (3, 2)
    assert got(mk(cache_interval=0)) == (0, 1) and got(mk(cache_interval=5, cache_levels=1)) == (5, 1)  # an argument wins
    assert got(S.DPMPP2MSampler(S.DDPMDiscretization(), S.VanillaCFG(), num_steps=3, device="cpu")) == (3, 2)
    for name, bad in (("SEVA_CACHE_INTERVAL", "two"), ("SEVA_CACHE_INTERVAL", "-1"), ("SEVA_CACHE_INTERVAL", "2.5"),
                      ("SEVA_CACHE_LEVELS", "0"), ("SEVA_CACHE_LEVELS", "4"), ("SEVA_CACHE_LEVELS", "deep")):
        with monkeypatch.context() as mp:
            mp.setenv(name, bad)
            with pytest.raises(ValueError):
                mk()
    for kw in (dict(cache_interval=-2), dict(cache_interval=2.0), dict(cache_interval=True), dict(cache_interval=2, cache_levels=0),
               dict(cache_interval=2, cache_levels=4), dict(cache_interval="x")):
        with pytest.raises(ValueError):
            mk(**kw)


def test_drivers_hand_the_values_to_every_window(cpu_sampler, monkeypatch):
    from seva import pipeline
    seen = []
    c2ws, Ks, lat, tok = _scene(43)

    def run(fn=pipeline.run_trajectory, **kw):
        del seen[:]
        res = fn(_fake_net, lat, c2ws, Ks, [0], clip_token=tok, T=21, num_steps=3, seed=23, device="cpu",
                 sampler_hook=lambda sm: seen.append((sm.cache_interval, sm.cache_levels)), **kw)
        return res

    plan = run()["plan"]
    n1, n2 = len(plan.pass1), len(plan.pass2)
    assert n1 >= 1 and n2 >= 1 and seen == [(0, 1)] * (n1 + n2)
    run(cache_interval=2)
    assert seen == [(2, 1)] * (n1 + n2)
    run(cache_interval=(3, 2), cache_levels=(1, 2))
    assert seen == [(3, 1)] * n1 + [(2, 2)] * n2
    run(cache_interval=(0, 4), cache_levels=3)
    assert seen == [(0, 3)] * n1 + [(4, 3)] * n2
    run(pipeline.run_views, cache_interval=2, cache_levels=2)
    assert seen and set(seen) == {(2, 2)}
    monkeypatch.setenv("SEVA_CACHE_INTERVAL", "5")
    run()
    assert seen == [(5, 1)] * (n1 + n2)
    run(cache_interval=0)
    assert seen == [(0, 1)] * (n1 + n2)
    # one window, directly
    win = plan.pass1[0]
    noise = torch.randn((len(win.slot_frame), 4, 8, 8), generator=torch.Generator().manual_seed(0))
    pipeline.run_window(win, {0: lat[0]}, _fake_net, c2ws, Ks, hw=(8, 8), num_steps=3, cfg=2.0, cfg_min=1.2, guider=1, camera_scale=2.0,
                        noise=noise, step_seed=1, clip_token=tok, device="cpu", cache_interval=2, cache_levels=3,
                        sampler_hook=lambda sm: seen.append(("window", sm.cache_interval, sm.cache_levels)))
    assert seen[-1] == ("window", 2, 3)


# ------------------------------------------------------------------------------------------------ whole-step graphs
@pytest.mark.parametrize("solver", ["euler", "dpmpp2m"])
def test_full_and_shallow_steps_take_distinct_graph_entries(cpu_sampler, monkeypatch, solver):
    from seva import _stepgraph
    S = cpu_sampler
    monkeypatch.setattr(_stepgraph, "StepGraph", FakeStepGraph)
    monkeypatch.setattr(S.EulerEDMSampler, "_whole_step_graph_eligible", lambda self, x: not self._step_graphs.disabled)
    steps, N, L = 7, 2, 2
    eager_net, net = Recorder(), Recorder()
    eager = _sampler(S, solver, steps, cache_interval=N, cache_levels=L)
    ref = _trajectory(eager, eager_net)
    sm = _sampler(S, solver, steps, cache_interval=N, cache_levels=L)
    sm._step_graphs.disabled = False
    got = _trajectory(sm, net)
    cache = sm._step_graphs
    assert torch.equal(got, ref) and net.levels == eager_net.levels == _expected(steps, N, L)
    # full steps 0 2 4 6: warm-up, capture, 2 further replays; shallow steps 1 3 5: warm-up, capture, 1 further replay
    assert sorted(cache.entries) == [0, L] and cache.captures == 2 and not cache.disabled
    full, shallow = cache.entries[0], cache.entries[L]
    assert full.graph is not shallow.graph and cache.graph is full.graph
    assert (full.graph.replays, shallow.graph.replays) == (3, 2)
    # a second trajectory through the same sampler reuses both
    ref2 = _trajectory(eager, Recorder(), seed=2)
    got2 = _trajectory(sm, net, seed=2)
    assert torch.equal(got2, ref2) and not torch.equal(ref2, ref)
    assert cache.captures == 2 and (full.graph.replays, shallow.graph.replays) == (3 + 4, 2 + 3)
    assert cache.entries[0] is full and cache.entries[L] is shallow
