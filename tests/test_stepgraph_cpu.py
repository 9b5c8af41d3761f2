"""The whole-step hipGraph protocol (`seva._stepgraph.StepGraphCache.run`) on the CPU: eager while not eligible, eager warm-up,
capture, replay, the capture-failed fallback -- first on the method itself, then through `EulerEDMSampler.sampler_step` for both
solvers and the three guiders.  `_stepgraph.StepGraph` is replaced by a stand-in that behaves like a capture: constructing it
records `fn` WITHOUT running it, calling it copies the inputs into static buffers, runs `fn` on those and returns one output
buffer that the next call overwrites.  The operators are tests/fake_ops.py, as in tests/test_solver_dpmpp2m_cpu.py."""
import warnings

import pytest
import torch

from test_pipeline_cpu import _patch_cpu
from test_solver_dpmpp2m_cpu import SCALE, SHAPE, _denoiser, _fake_cfg_multistep

STEPS = 4


class FakeStepGraph:
    def __init__(self, fn, inputs):
        self.fn = fn
        self.static_in = [torch.empty_like(t) for t in inputs]
        self.static_out = None
        self.replays = 0

    def __call__(self, *inputs):
        for s, t in zip(self.static_in, inputs):
            s.copy_(t)
        out = self.fn(*self.static_in)
        if self.static_out is None:
            self.static_out = torch.empty_like(out)
        self.static_out.copy_(out)
        self.replays += 1
        return self.static_out


class FailingStepGraph:
    def __init__(self, fn, inputs):
        raise RuntimeError("operation not permitted when stream is capturing")


@pytest.fixture
def sg(monkeypatch):
    from seva import _stepgraph
    monkeypatch.setattr(_stepgraph, "StepGraph", FakeStepGraph)
    return _stepgraph


def _step():
    """(fn, log): fn(a, b) = 2 a + b, and per call whether the network was forced eager"""
    from seva import _native
    log = []

    def fn(a, b):
        log.append(_native.network_eager_forced())
        return 2 * a + b

    return fn, log


def _inputs(i):
    return torch.full((3,), float(i)), torch.arange(3.0)


def test_not_eligible_runs_fn_and_leaves_the_cache_alone(sg):
    cache, (fn, log) = sg.StepGraphCache(), _step()
    for i in range(3):
        a, b = _inputs(i)
        assert torch.equal(cache.run(("k", 1), fn, (a, b), eligible=False, keep=lambda: "kept"), 2 * a + b)
    assert log == [False] * 3
    assert (cache.key, cache.state, cache.graph, cache.keep, cache.disabled, cache.captures) == (None, 0, None, None, False, 0)


def test_warm_up_capture_replay(sg):
    cache, (fn, log) = sg.StepGraphCache(), _step()
    kept, reads = object(), []

    def keep():
        reads.append(cache.captures)
        return kept

    key = ("k", 1.5, fn)
    a, b = _inputs(1)
    r1 = cache.run(key, fn, (a, b), eligible=True, keep=keep)
    # first call of a key: the real step, eagerly, with the network-only graph held off; nothing captured, nothing kept
    assert log == [True] and torch.equal(r1, 2 * a + b)
    assert cache.state == 1 and cache.graph is None and cache.captures == 0 and cache.keep is None and not reads
    a, b = _inputs(2)
    r2 = cache.run(key, fn, (a, b), eligible=True, keep=keep)
    # second call: captured (construction does not run fn) and replayed once; `keep` read once, after the capture counted
    assert log == [True, False] and torch.equal(r2, 2 * a + b)
    assert cache.captures == 1 and cache.graph.replays == 1 and cache.keep is kept and reads == [1]
    a, b = _inputs(3)
    r3 = cache.run(key, fn, (a, b), eligible=True, keep=keep)
    assert cache.captures == 1 and cache.graph.replays == 2 and reads == [1] and torch.equal(r3, 2 * a + b)
    # the caller never gets the graph's output buffer: an earlier result survives the next replay
    out = cache.graph.static_out
    assert all(r is not out and r.data_ptr() != out.data_ptr() for r in (r2, r3))
    assert torch.equal(r2, 2 * _inputs(2)[0] + b)
    # an equal key built anew is the same key
    cache.run(("k", 1.5, fn), fn, (a, b), eligible=True, keep=keep)
    assert cache.captures == 1 and cache.graph.replays == 3


def test_another_key_starts_over(sg):
    cache, (fn, log) = sg.StepGraphCache(), _step()
    a, b = _inputs(1)
    for _ in range(3):
        cache.run(("k", 1), fn, (a, b), eligible=True, keep=lambda: "kept")
    assert cache.captures == 1 and cache.graph.replays == 2 and cache.keep == "kept"
    del log[:]
    r = cache.run(("k", 2), fn, (a, b), eligible=True, keep=lambda: "kept")
    assert log == [True] and torch.equal(r, 2 * a + b)  # warm-up again
    assert cache.state == 1 and cache.graph is None and cache.keep is None and cache.captures == 1
    cache.run(("k", 2), fn, (a, b), eligible=True)  # and a capture of its own; no `keep` given: nothing held
    assert cache.captures == 2 and cache.graph.replays == 1 and cache.keep is None


def test_failed_capture_disables_and_runs_eagerly(sg, monkeypatch):
    monkeypatch.setattr(sg, "StepGraph", FailingStepGraph)
    cache, (fn, log) = sg.StepGraphCache(), _step()
    a, b = _inputs(1)
    cache.run(("k",), fn, (a, b), eligible=True, keep=lambda: "kept")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        r = cache.run(("k",), fn, (a, b), eligible=True, keep=lambda: "kept")
    assert len(caught) == 1 and caught[0].category is RuntimeWarning
    assert str(caught[0].message) == ("seva: whole-step hipGraph capture failed (RuntimeError: operation not permitted when stream "
                                      "is capturing); falling back to eager steps")
    assert torch.equal(r, 2 * a + b) and log == [True, False]
    assert cache.disabled and (cache.key, cache.state, cache.graph, cache.keep, cache.captures) == (None, 0, None, None, 0)
    # `disabled` is part of the sampler's eligibility: every later call is eager
    for _ in range(2):
        assert torch.equal(cache.run(("k",), fn, (a, b), eligible=not cache.disabled, keep=lambda: "kept"), 2 * a + b)
    assert log == [True, False, False, False] and (cache.key, cache.state, cache.graph, cache.captures) == (None, 0, None, 0)


# ------------------------------------------------------------------------------------------------ through sampler_step
@pytest.fixture
def cpu_sampler(sg, monkeypatch):
    """fake operators, the stand-in graph, and every condition of the eligibility predicate but `disabled` taken as met"""
    import seva.ops as ops
    from seva import sampling as S
    monkeypatch.delenv("SEVA_SOLVER", raising=False)
    _patch_cpu(monkeypatch)
    monkeypatch.setattr(ops, "cfg_multistep", _fake_cfg_multistep, raising=False)
    monkeypatch.setattr(S.EulerEDMSampler, "_whole_step_graph_eligible", lambda self, x: not self._step_graphs.disabled)
    return S


def _views():
    from seva import synthetic as synth
    T = SHAPE[0]
    mask = torch.zeros(T, dtype=torch.bool)
    mask[0] = True
    return {"c2w": synth.orbit_c2w(T), "K": synth.default_K(T), "input_frame_mask": mask}


def _guider(S, kind):
    return {"vanilla": S.VanillaCFG, "multiview": lambda: S.MultiviewCFG(1.2),
            "temporal": lambda: S.MultiviewTemporalCFG(SHAPE[0], 1.2)}[kind]()


def _sampler(S, solver, kind, graphs):
    sm = S.EulerEDMSampler(S.DDPMDiscretization(), _guider(S, kind), num_steps=STEPS, verbose=False, device="cpu", solver=solver,
                           s_churn=0.5 if solver == "euler" else 0.0)  # gamma > 0: the drawn eps reaches the result
    sm._step_graphs.disabled = not graphs
    return sm


def _trajectory(sm, kwargs, seed):
    g = torch.Generator().manual_seed(seed)
    sm.noise_fn = lambda x: torch.randn(x.shape, generator=g)
    x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(100 + seed))
    return sm(_denoiser, x, SCALE, {}, {}, verbose=False, **kwargs)


@pytest.mark.parametrize("solver", ["euler", "dpmpp2m"])
def test_failed_capture_in_a_trajectory_gives_the_eager_result(cpu_sampler, sg, monkeypatch, solver):
    S = cpu_sampler
    ref = _trajectory(_sampler(S, solver, "multiview", False), _views(), 1)
    monkeypatch.setattr(sg, "StepGraph", FailingStepGraph)
    sm = _sampler(S, solver, "multiview", True)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = _trajectory(sm, _views(), 1)
    assert [w.category for w in caught] == [RuntimeWarning] and "whole-step hipGraph capture failed" in str(caught[0].message)
    assert torch.equal(got, ref) and sm._step_graphs.disabled and sm._step_graphs.captures == 0 and sm._step_graphs.graph is None


@pytest.mark.parametrize("kind", ["vanilla", "multiview", "temporal"])
@pytest.mark.parametrize("solver", ["euler", "dpmpp2m"])
def test_graphed_trajectory_equals_the_eager_one(cpu_sampler, solver, kind):
    S = cpu_sampler
    kwargs = {} if kind == "vanilla" else _views()
    eager, graphed = _sampler(S, solver, kind, False), _sampler(S, solver, kind, True)
    ref = _trajectory(eager, kwargs, 1)
    assert eager._step_graphs.captures == 0 and eager._step_graphs.graph is None and torch.isfinite(ref).all()
    got = _trajectory(graphed, kwargs, 1)
    cache = graphed._step_graphs
    assert torch.equal(got, ref)
    assert cache.captures == 1 and cache.graph.replays == STEPS - 1 and not cache.disabled
    # what the graph reads by address is held by the cache: the guider's rule entry of this trajectory, where it has one
    assert cache.keep is getattr(graphed.guider, "_rule_cache", None) and (cache.keep is None) == (kind == "vanilla")
    if solver != "dpmpp2m":
        return
    # the key holds the history buffer: a second trajectory on the same sampler replays the same graph from its first step on
    ref2 = _trajectory(eager, kwargs, 2)
    kept = cache.keep
    assert torch.equal(_trajectory(graphed, kwargs, 2), ref2) and not torch.equal(ref2, ref)
    assert cache.captures == 1 and cache.graph.replays == 2 * STEPS - 1 and cache.keep is kept
    # and history left behind, NaN included, never reaches the next trajectory
    graphed._ms_den.fill_(float("nan"))
    assert torch.equal(_trajectory(graphed, kwargs, 1), ref) and cache.captures == 1
