"""The host arithmetic that `seva.sampling` and `seva.pipeline` expose as functions of their own: the step schedule
(`sampling.step_kinds`), the one resolver of the sampler's options (`sampling.resolve_options`) with the per-pass rule of the drivers
(`sampling.per_pass_options`), and the ownership rule of the first pass (`pipeline.first_pass_owner`).  No operator runs here."""
import pytest
import torch

INF = float("inf")
ENV = ("SEVA_SOLVER", "SEVA_CACHE_INTERVAL", "SEVA_CACHE_LEVELS", "SEVA_GUIDANCE_INTERVAL", "SEVA_GUIDANCE_RESCALE")
STEPS = 10
INTERVAL = (3.0, 25.0)  # tests/test_guidance_cpu.py: both bounds lie between values of the 10-step schedule, steps 3..7 are guided


def _sigmas():
    from seva import sampling as S
    return S.DDPMDiscretization()(STEPS)


def _kinds(letters, guided, levels):
    out = []
    for letter, g in zip(letters.split(), guided):
        out.append({**({"shallow": levels} if letter == "S" else {}), **({} if g else {"guided": False})})
    return out


# ------------------------------------------------------------------------------------------------ schedule
def test_step_kinds_of_the_ten_step_case():
    from seva.sampling import step_kinds
    sig = _sigmas()
    guided = [3 <= i <= 7 for i in range(STEPS)]
    # step 8: full where the guided flag flips (step 3 is full by i % 3 anyway); step 9: the last
    assert step_kinds(sig, 3, 2, INTERVAL) == _kinds("F S S F S S F S F F", guided, 2)
    assert step_kinds(sig, 3, 2, INTERVAL)[4] == {"shallow": 2} and step_kinds(sig, 3, 2, INTERVAL)[1] == {"shallow": 2, "guided": False}
    # each feature alone
    assert step_kinds(sig, 3, 2, None) == _kinds("F S S F S S F S S F", [True] * STEPS, 2)
    assert step_kinds(sig, 0, 2, INTERVAL) == _kinds("F F F F F F F F F F", guided, 2)
    # a boundary that does not fall on a multiple of the interval: (5, 40) guides steps 2..6
    assert step_kinds(sig, 3, 1, (5.0, 40.0)) == _kinds("F S F F S S F F S F", [2 <= i <= 6 for i in range(STEPS)], 1)


def test_step_kinds_with_everything_off_adds_no_keyword():
    from seva.sampling import step_kinds
    sig = _sigmas()
    assert len(sig) == STEPS + 1
    for levels in (1, 3):
        assert step_kinds(sig, 0, levels, None) == [{}] * STEPS
    assert step_kinds(sig, 0, 1, (0.0, INF)) == [{}] * STEPS  # an interval that holds every sigma
    assert step_kinds(sig[-2:], 3, 1, None) == [{}]             # one step: the first and the last


def test_step_kinds_upper_bound_inclusive_lower_bound_exclusive():
    """The sides that tests/test_guidance_cpu.py asserts through the sampler, on the function: a bound exactly on a schedule sigma,
    one fp32 ulp off it, and within half an fp32 ulp of it (the comparison runs in the sigmas' dtype)."""
    from seva.sampling import step_kinds
    sig = _sigmas()
    s3, s7 = float(sig[3]), float(sig[7])
    for interval, want in (((3.0, s3), [3, 4, 5, 6, 7]),
                           ((s7, 25.0), [3, 4, 5, 6]),
                           ((3.0, float(torch.nextafter(sig[3], sig[4]))), [4, 5, 6, 7]),
                           ((3.0, s3 * (1 - 2.0 ** -26)), [3, 4, 5, 6, 7])):
        got = step_kinds(sig, 0, 1, interval)
        assert [i for i, k in enumerate(got) if k.get("guided", True)] == want, interval
        assert all(k in ({}, {"guided": False}) for k in got)


# ------------------------------------------------------------------------------------------------ resolver
def _opts(solver="euler", cache_interval=0, cache_levels=1, guidance_interval=None, guidance_rescale=0.0):
    return dict(solver=solver, cache_interval=cache_interval, cache_levels=cache_levels, guidance_interval=guidance_interval,
                guidance_rescale=guidance_rescale)


RESOLVE = [
    # (arguments, environment, resolved options or the exception)
    ({}, {}, _opts()),
    (dict(cache_interval=4), {}, _opts(cache_interval=4)),
    (dict(cache_interval=2, cache_levels=3), {}, _opts(cache_interval=2, cache_levels=3)),
    (dict(cache_interval=1, cache_levels=2), {}, _opts(cache_levels=2)),                      # 0 and 1 are both "off"
    (dict(cache_interval=None, cache_levels=3), {}, _opts(cache_levels=3)),
    ({}, {"SEVA_CACHE_INTERVAL": "3"}, _opts(cache_interval=3)),
    (dict(cache_levels=2), {"SEVA_CACHE_INTERVAL": "3"}, _opts(cache_interval=3, cache_levels=2)),   # depth: the argument where its variable is unset
    ({}, {"SEVA_CACHE_INTERVAL": "3", "SEVA_CACHE_LEVELS": "2"}, _opts(cache_interval=3, cache_levels=2)),
    (dict(cache_levels=3), {"SEVA_CACHE_INTERVAL": "3", "SEVA_CACHE_LEVELS": "2"}, _opts(cache_interval=3, cache_levels=2)),
    (dict(cache_levels=3), {"SEVA_CACHE_INTERVAL": "3", "SEVA_CACHE_LEVELS": ""}, _opts(cache_interval=3, cache_levels=3)),
    ({}, {"SEVA_CACHE_LEVELS": "2"}, _opts(cache_levels=2)),                                  # read with the interval's variable, which is unset: off
    (dict(cache_interval=0), {"SEVA_CACHE_INTERVAL": "3", "SEVA_CACHE_LEVELS": "2"}, _opts()),  # an argument wins, and SEVA_CACHE_LEVELS is ignored
    (dict(cache_interval=5, cache_levels=1), {"SEVA_CACHE_INTERVAL": "3", "SEVA_CACHE_LEVELS": "2"}, _opts(cache_interval=5)),
    (dict(cache_interval=5), {"SEVA_CACHE_LEVELS": "4"}, _opts(cache_interval=5)),            # not even parsed
    ({}, {"SEVA_CACHE_INTERVAL": ""}, _opts()),
    ({}, {"SEVA_CACHE_INTERVAL": "1"}, _opts()),
    ({}, {"SEVA_SOLVER": "dpmpp2m"}, _opts(solver="dpmpp2m")),
    ({}, {"SEVA_SOLVER": ""}, _opts()),                                                       # empty: unset
    (dict(solver="euler"), {"SEVA_SOLVER": "dpmpp2m"}, _opts()),
    (dict(solver="dpmpp2m"), {"SEVA_SOLVER": "heun"}, _opts(solver="dpmpp2m")),
    (dict(guidance_interval=(0.3, 5)), {}, _opts(guidance_interval=(0.3, 5.0))),
    (dict(guidance_rescale=0.7), {}, _opts(guidance_rescale=0.7)),
    ({}, {"SEVA_GUIDANCE_INTERVAL": "0.3,5"}, _opts(guidance_interval=(0.3, 5.0))),
    ({}, {"SEVA_GUIDANCE_INTERVAL": "0.3,5", "SEVA_GUIDANCE_RESCALE": "0.7"}, _opts(guidance_interval=(0.3, 5.0), guidance_rescale=0.7)),
    (dict(guidance_interval=(0, INF)), {"SEVA_GUIDANCE_INTERVAL": "0.3,5", "SEVA_GUIDANCE_RESCALE": "0.7"},
     _opts(guidance_interval=(0.0, INF), guidance_rescale=0.7)),
    (dict(guidance_rescale=0), {"SEVA_GUIDANCE_INTERVAL": "0.3,5", "SEVA_GUIDANCE_RESCALE": "0.7"}, _opts(guidance_interval=(0.3, 5.0))),
    (dict(guidance_interval=(1, 2), guidance_rescale=0.25), {"SEVA_GUIDANCE_INTERVAL": "0.3,5", "SEVA_GUIDANCE_RESCALE": "0.7"},
     _opts(guidance_interval=(1.0, 2.0), guidance_rescale=0.25)),
    ({}, {"SEVA_GUIDANCE_INTERVAL": "", "SEVA_GUIDANCE_RESCALE": ""}, _opts()),
    (dict(solver="dpmpp2m", cache_interval=3, cache_levels=2, guidance_interval="3,25", guidance_rescale="1"),
     {"SEVA_SOLVER": "euler", "SEVA_CACHE_INTERVAL": "2", "SEVA_CACHE_LEVELS": "3", "SEVA_GUIDANCE_INTERVAL": "1,2", "SEVA_GUIDANCE_RESCALE": "0"},
     _opts("dpmpp2m", 3, 2, (3.0, 25.0), 1.0)),
    # errors keep their type
    (dict(solver="heun"), {}, ValueError),
    (dict(solver=""), {}, ValueError),                                                        # only the VARIABLE may be empty
    (dict(solver=("euler", "dpmpp2m")), {}, ValueError),                                      # one value: no per-pass pair
    ({}, {"SEVA_SOLVER": "heun"}, ValueError),
    ({}, {"SEVA_CACHE_INTERVAL": "two"}, ValueError),
    ({}, {"SEVA_CACHE_INTERVAL": "3", "SEVA_CACHE_LEVELS": "4"}, ValueError),
    (dict(cache_interval=2, cache_levels=0), {}, ValueError),
    (dict(cache_interval=True), {}, ValueError),
    ({}, {"SEVA_GUIDANCE_INTERVAL": "5,0.3"}, ValueError),
    ({}, {"SEVA_GUIDANCE_RESCALE": "2"}, ValueError),
    (dict(guidance_interval=3.0), {}, ValueError),
    (dict(guidance_rescale=1.5), {}, ValueError),
]


@pytest.mark.parametrize("args,env,want", RESOLVE)
def test_resolve_options(monkeypatch, args, env, want):
    from seva import sampling as S
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    if isinstance(want, dict):
        got = S.resolve_options(**args)
        assert got == want and list(got) == list(want)
        assert type(got["cache_interval"]) is int and type(got["cache_levels"]) is int and type(got["guidance_rescale"]) is float
    else:
        with pytest.raises(want):
            S.resolve_options(**args)


def test_the_sampler_holds_what_the_resolver_returns(monkeypatch):
    from seva import sampling as S
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SEVA_CACHE_INTERVAL", "3")
    monkeypatch.setenv("SEVA_GUIDANCE_RESCALE", "0.5")
    args = dict(solver="dpmpp2m", cache_levels=2, guidance_interval=(0.3, 5))
    sm = S.EulerEDMSampler(S.DDPMDiscretization(), S.VanillaCFG(), num_steps=3, device="cpu", **args)
    assert {k: getattr(sm, k) for k in _opts()} == S.resolve_options(**args) == _opts("dpmpp2m", 3, 2, (0.3, 5.0), 0.5)
    sm.guidance_rescale = 0.25  # plain attributes: assignable after construction
    assert sm.guidance_rescale == 0.25
    with pytest.raises(ValueError, match="s_churn"):  # the solver's own check stays in the constructor
        S.EulerEDMSampler(S.DDPMDiscretization(), S.VanillaCFG(), num_steps=3, device="cpu", solver="dpmpp2m", s_churn=0.5)


def test_per_pass_options():
    from seva.sampling import per_pass, per_pass_options
    assert per_pass(21) == (21, 21) and per_pass((96, 21)) == (96, 21) and per_pass([3.0, 2.0]) == (3.0, 2.0) and per_pass(None) == (None, None)
    with pytest.raises(AssertionError):
        per_pass((1, 2, 3))
    default = dict(solver=None, cache_interval=None, cache_levels=1, guidance_interval=None, guidance_rescale=None)
    assert per_pass_options() == (default, default)
    a, b = per_pass_options(solver="dpmpp2m", cache_interval=(3, 2), cache_levels=(1, 2), guidance_rescale=(0.0, 0.5))
    assert a == dict(default, solver="dpmpp2m", cache_interval=3, cache_levels=1, guidance_rescale=0.0)
    assert b == dict(default, solver="dpmpp2m", cache_interval=2, cache_levels=2, guidance_rescale=0.5)
    # the interval: a 2-tuple whose elements are each None, a tuple or a string is a pair; anything else is one value for both passes
    for value, want in ((((0.5, 3), None), ((0.5, 3), None)), ((None, (1, INF)), (None, (1, INF))), (("0.3,5", (0.5, 3)), ("0.3,5", (0.5, 3))),
                        ((None, None), (None, None)), ([[0.3, 5], "1,2"], ([0.3, 5], "1,2")),
                        ((0.3, 5), ((0.3, 5), (0.3, 5))), ("0.3,5", ("0.3,5", "0.3,5")), (None, (None, None)),
                        ((5, 0.3), ((5, 0.3), (5, 0.3))), ((0.3, 5, 7), ((0.3, 5, 7), (0.3, 5, 7))), ((None, 5), ((None, 5), (None, 5)))):
        a, b = per_pass_options(guidance_interval=value)
        assert (a["guidance_interval"], b["guidance_interval"]) == want, value
    # `solver` stays one value: a pair reaches the resolver as it is, and is refused there
    a, b = per_pass_options(solver=("euler", "dpmpp2m"))
    assert a["solver"] == b["solver"] == ("euler", "dpmpp2m")
    with pytest.raises(AssertionError):
        per_pass_options(cache_interval=(1, 2, 3))


# ------------------------------------------------------------------------------------------------ ownership of the first pass
def _plans():
    from seva import pipeline
    from seva import synthetic as synth
    c2ws = synth.orbit_c2w(43)
    return {"two-pass, serial": pipeline.plan_trajectory(c2ws, [0], T=21),
            "two-pass, independent": pipeline.plan_trajectory(c2ws, [0], T=21, first_pass_strategy="gt"),
            "one-pass, serial": pipeline.plan_views(c2ws, [0], T=21, chunk_strategy="gt-nearest"),
            "one-pass, independent": pipeline.plan_views(c2ws, [0], T=21)}


@pytest.mark.parametrize("world", [1, 2, 4])
@pytest.mark.parametrize("split1", [False, True])
def test_first_pass_owner(world, split1):
    from seva.distributed import shard_windows
    from seva.pipeline import first_pass_owner
    plans = _plans()
    assert [p.pass1_serial for p in plans.values()] == [True, False, True, False]
    assert len(plans["one-pass, independent"].pass1) == 3 and len(plans["one-pass, serial"].pass1) == 3  # more windows than some worlds have ranks
    for name, plan in plans.items():
        n = len(plan.pass1)
        owners = [first_pass_owner(plan, i, world, split1) for i in range(n)]
        # every window has exactly one owner, a rank of the world
        assert all(type(o) is int and 0 <= o < world for o in owners), (name, owners)
        counts = [sum(len(plan.pass1[i].target_ids) for i in range(n) if owners[i] == r) for r in range(world)]
        assert sum(counts) == len(plan.anchor_ids), (name, counts)
        if plan.pass1_serial or split1 or world == 1:
            assert owners == [0] * n, name  # the pass runs in one place: rank 0 publishes (under split1, rank 1 holds the same bits)
        else:
            for r in range(world):
                assert [i for i in range(n) if owners[i] == r] == shard_windows(n, r, world), (name, r)
