"""The stochastic Euler sampler (s_churn > 0) on the CPU, against goldens recorded from the reference's own
`EulerEDMSampler.__call__` (tests/golden/g14_churn_analytic.npz, oracle/make_goldens_churn.py): which gamma reaches each
`sampler_step` (the window comparison, bounds within half an fp32 ulp of a schedule sigma included), the output, and the counters
of the whole-step graph protocol when gamma changes inside a trajectory.  The operators are tests/fake_ops.py and the capture is the
stand-in of tests/test_stepgraph_cpu.py; the cases, the analytic denoiser and the fp64 restatement are tests/churn_cases.py.

Bound on every rel-L2 against the golden: 10 x the largest `ref_vs_fp64` the generator stored (the reference's fp32 output against
the fp64 restatement fed the fp32 per-step scalars; 1.11e-7, so 1.11e-6) -- the factor tests/test_solver_dpmpp2m_gpu.py uses over
its fp32 emulation.  Measured on the CPU: 0 where s_noise = 1 (the same bits), up to 8.5e-8 where it is not: the sampler folds
s_noise into the noise scale, the reference into eps (profiles/sampler_churn.log)."""
import pytest
import torch

import churn_cases as C
from conftest import load_golden
from test_stepgraph_cpu import FakeStepGraph, cpu_sampler, sg  # noqa: F401  (fixtures, not copied into a conftest)

CASE_GUIDER = [(c, k) for c in C.CASES for k in C.GUIDERS]
IDS = [f"{c}-{k}" for c, k in CASE_GUIDER]


@pytest.fixture(scope="module")
def gold():
    return load_golden(C.GOLDEN)


def bound_of(g):
    return 10.0 * max(float(g[f"{c}__{k}__ref_vs_fp64"]) for c, k in CASE_GUIDER)


def views_of(g):
    return {"c2w": g["c2w"], "K": g["K"], "input_frame_mask": g["mask"].bool()}


def test_golden_is_the_one_these_cases_generate(gold):
    """The fixture was recorded with the settings, inputs and eps that tests/churn_cases.py states (a stale file would make every
    comparison below meaningless), and holds what the bound is derived from."""
    from seva import sampling as S
    from seva import synthetic as synth
    disc = S.DDPMDiscretization()
    v = C.views(synth)
    assert torch.equal(gold["noise"], C.noise()) and all(torch.equal(views_of(gold)[k], v[k]) for k in v)
    for name in C.CASES:
        st = C.settings(name, disc)
        assert all(float(gold[f"{name}__{k}"]) == st[k] for k in st), name
        assert torch.equal(gold[f"{name}__eps"], torch.stack(C.eps_list(st["steps"])))
    # the two edge bounds are no schedule sigma as doubles, and round to one in fp32
    for name, key, i in (("edge_hi", "s_tmax", 2), ("edge_lo", "s_tmin", 5)):
        st = C.settings(name, disc)
        s = disc(st["steps"])[i]
        assert st[key] != float(s) and torch.tensor(st[key], dtype=torch.float32) == s
    assert 0 < bound_of(gold) < 1e-5


class Recording:
    """Mixin: records the gamma of every `sampler_step` call (an override in a subclass, the GradioTrackedSampler pattern)."""

    def sampler_step(self, sigma, next_sigma, denoiser, x, scale, cond, uc, gamma=0.0, **kw):
        self.__dict__.setdefault("gammas", []).append(gamma)
        return super().sampler_step(sigma, next_sigma, denoiser, x, scale, cond, uc, gamma, **kw)


def _sampler(S, gold, case, kind, graphs=False, **over):
    st = C.settings(case, S.DDPMDiscretization())
    st.update(over)

    class Sampler(Recording, S.EulerEDMSampler):
        pass

    sm = Sampler(S.DDPMDiscretization(), C.make_guider(S, kind), num_steps=st["steps"], verbose=False, device="cpu",
                 s_churn=st["s_churn"], s_tmin=st["s_tmin"], s_tmax=st["s_tmax"], s_noise=st["s_noise"])
    sm._step_graphs.disabled = not graphs
    return sm


def _trajectory(sm, gold, case, kwargs, eps=None):
    it = iter(gold[f"{case}__eps"] if eps is None else eps)
    sm.noise_fn = lambda x: next(it).clone()
    return sm(C.denoiser, gold["noise"].clone(), C.SCALE, {}, {}, verbose=False, **kwargs)


@pytest.mark.parametrize("case,kind", CASE_GUIDER, ids=IDS)
def test_gamma_sequence_and_output_equal_the_reference(cpu_sampler, gold, case, kind):
    """The window comparison: the sampler hands `sampler_step` exactly the gammas the reference handed its own, on every case and
    with every guider; and the trajectory lands on the reference's output within the bound."""
    S = cpu_sampler
    sm = _sampler(S, gold, case, kind)
    got = _trajectory(sm, gold, case, C.guider_kwargs(kind, views_of(gold)))
    want = [float(v) for v in gold[f"{case}__{kind}__gamma"]]
    assert all(isinstance(v, float) for v in sm.gammas) and sm.gammas == want, (sm.gammas, want)
    rel, bound = C.rel_l2(got, gold[f"{case}__{kind}__y"]), bound_of(gold)
    print(f"{case} {kind}: CPU (emulated operators) vs reference golden rel-L2 {rel:.3e}, bound {bound:.3e}; "
          f"golden vs fp64 restatement {float(gold[f'{case}__{kind}__ref_vs_fp64']):.3e}")
    assert got.dtype == torch.float32 and rel <= bound


def test_restatement_is_fed_what_the_reference_formed(gold):
    """`churn_cases.step_scalars` gives bit for bit the fp32 sigma_hat that each denoiser call of the reference saw."""
    from seva import sampling as S
    for case, kind in CASE_GUIDER:
        sigmas = S.DDPMDiscretization()(C.CASES[case][0])
        for i, gamma in enumerate(gold[f"{case}__{kind}__gamma"]):
            assert torch.equal(C.step_scalars(sigmas, i, float(gamma), 1)[0], gold[f"{case}__{kind}__sigma_hat"][i:i + 1]), (case, i)


def test_the_golden_tells_the_three_mutants_apart(gold):
    """Without the sampler: the fp64 restatement with (i) s_noise ignored, (ii) gamma ignored, (iii) the noise scale
    sigma_hat - sigma in place of sqrt(sigma_hat^2 - sigma^2) is at least 100 x the bound away from the golden on at least one
    case -- and (i), which cannot show where s_noise = 1, on each of `window`, `capped` and `inner`."""
    from seva import sampling as S
    bound = bound_of(gold)
    v = views_of(gold)
    sep = {m: {} for m in C.MUTANTS}
    for case, kind in CASE_GUIDER:
        st = C.settings(case, S.DDPMDiscretization())
        args = (gold["noise"], gold[f"{case}__eps"], S.DDPMDiscretization()(st["steps"]), gold[f"{case}__{kind}__gamma"], st["s_noise"],
                C.frame_scale(kind, v))
        assert C.rel_l2(gold[f"{case}__{kind}__y"], C.restate_fp64(*args)) <= bound
        for m in C.MUTANTS:
            sep[m][case, kind] = C.rel_l2(C.restate_fp64(*args, mutant=m), gold[f"{case}__{kind}__y"])
    for m in C.MUTANTS:
        per_case = {c: min(sep[m][c, k] for k in C.GUIDERS) for c in C.CASES}
        print(f"mutant {m}: rel-L2 from the golden, smallest over the guiders, in units of the bound "
              f"{ {c: round(r / bound, 1) for c, r in per_case.items()} }")
        assert max(per_case.values()) >= 100 * bound, (m, per_case)
    for case in ("window", "capped", "inner"):
        assert all(sep["s_noise_ignored"][case, k] >= 100 * bound for k in C.GUIDERS), case
    assert all(sep["s_noise_ignored"]["all", k] <= bound for k in C.GUIDERS)  # s_noise = 1: nothing to ignore


@pytest.mark.parametrize("case,kind", CASE_GUIDER, ids=IDS)
def test_protocol_counters_follow_the_gamma_runs(cpu_sampler, gold, case, kind):
    """gamma is part of the whole-step graph key: every maximal run of equal gamma (length L) costs one eager warm-up, one capture
    if L >= 2, and L - 1 replays.  Expected counters come from the GOLDEN's gamma sequence; the result is the eager run's, bit for
    bit.  A second trajectory on the same sampler continues the count: its first key equals the last key of the first trajectory
    exactly where the two gammas are equal."""
    S = cpu_sampler
    kwargs = C.guider_kwargs(kind, views_of(gold))
    gammas = [float(v) for v in gold[f"{case}__{kind}__gamma"]]
    ref = _trajectory(_sampler(S, gold, case, kind), gold, case, kwargs)
    sm = _sampler(S, gold, case, kind, graphs=True)
    cache = sm._step_graphs
    warm = []
    real_run = cache.run

    def run(key, fn, inputs, *, eligible, keep=None):
        warm.append(eligible and (cache.key is None or not cache._same(cache.key, key)))
        return real_run(key, fn, inputs, eligible=eligible, keep=keep)

    cache.run = run
    for n in (1, 2):
        got = _trajectory(sm, gold, case, kwargs)
        warmups, captures, live = C.expected_counters(gammas * n)
        print(f"{case} {kind}, after trajectory {n}: warm-ups {sum(warm)}, captures {cache.captures}, "
              f"replays of the live graph {cache.graph.replays if cache.graph else None}; runs {C.runs_of(gammas * n)}")
        assert torch.equal(got, ref) and not cache.disabled
        assert (sum(warm), cache.captures) == (warmups, captures)
        assert (cache.graph.replays if cache.graph is not None else None) == live
        assert isinstance(cache.graph, FakeStepGraph) or live is None
    if gammas[0] != gammas[-1]:
        assert cache.captures > C.expected_counters(gammas)[1]  # the second trajectory captured again


def test_dpmpp2m_with_churn_still_raises(cpu_sampler):
    S = cpu_sampler
    for cls, kw in ((S.EulerEDMSampler, {"solver": "dpmpp2m"}), (S.DPMPP2MSampler, {})):
        with pytest.raises(ValueError):
            cls(S.DDPMDiscretization(), S.VanillaCFG(), num_steps=4, device="cpu", s_churn=1e-3, **kw)
