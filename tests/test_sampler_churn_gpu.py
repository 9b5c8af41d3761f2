"""The stochastic Euler sampler (s_churn > 0) on the device: `ops.add_noise` with a noise scale that is not ~0, sigma_hat in the
nearest-sigma lookup, and the whole-step hipGraph across key changes (gamma is part of the key, so a trajectory that enters or
leaves [s_tmin, s_tmax] warms up and captures again).  Goldens are recorded from the reference's own `EulerEDMSampler.__call__`
(oracle/make_goldens_churn.py); cases, analytic denoiser and fp64 restatement are tests/churn_cases.py, as on the CPU.

Bounds: analytic cases, rel-L2 <= 10 x the largest `ref_vs_fp64` stored in the golden (1.11e-7 -> 1.11e-6; measured on the device
7.7e-8 ... 1.14e-7 against the golden and 7.4e-8 ... 1.11e-7 against the restatement); the tiny-network loop, `NET_TOL` of
tests/test_model_gpu.py (measured 4.5e-4); graph against eager, bit for bit.  All figures: profiles/sampler_churn.log."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import churn_cases as C  # noqa: E402
from conftest import load_golden, rel_l2  # noqa: E402
from test_model_gpu import NET_TOL, dev, tiny  # noqa: E402,F401  (module-scoped fixtures, not copied into a conftest)
from test_sampler_churn_cpu import CASE_GUIDER, IDS, Recording, bound_of, views_of  # noqa: E402

T, HW = C.TINY["T"], C.TINY["hw"]


@pytest.fixture(scope="module")
def gold():
    return load_golden(C.GOLDEN)


@pytest.fixture(scope="module")
def device_runs(dev, gold):
    """(case, guider) -> (output on the host, gammas handed to sampler_step, (captures, live replays)), each computed once."""
    from seva import sampling as S
    done = {}

    def get(case, kind):
        if (case, kind) not in done:
            st = C.settings(case, S.DDPMDiscretization())

            class Sampler(Recording, S.EulerEDMSampler):
                pass

            sm = Sampler(S.DDPMDiscretization(), C.make_guider(S, kind), num_steps=st["steps"], verbose=False, device=dev,
                         s_churn=st["s_churn"], s_tmin=st["s_tmin"], s_tmax=st["s_tmax"], s_noise=st["s_noise"])
            it = iter(gold[f"{case}__eps"])
            sm.noise_fn = lambda x: next(it).to(x.device)
            kw = {k: v.to(dev) for k, v in C.guider_kwargs(kind, views_of(gold)).items()}
            y = sm(C.denoiser_on(dev), gold["noise"].to(dev), C.SCALE, {}, {}, verbose=False, **kw).cpu()
            cache = sm._step_graphs
            done[case, kind] = (y, sm.gammas, (cache.captures, cache.graph.replays if cache.graph is not None else None), cache.disabled)
        return done[case, kind]

    return get


@pytest.mark.parametrize("case,kind", CASE_GUIDER, ids=IDS)
def test_analytic_cases_against_the_reference_golden(device_runs, gold, case, kind, monkeypatch):
    monkeypatch.delenv("SEVA_SOLVER", raising=False)
    y, gammas, counters, disabled = device_runs(case, kind)
    want = [float(v) for v in gold[f"{case}__{kind}__gamma"]]
    rel, bound = rel_l2(y, gold[f"{case}__{kind}__y"]), bound_of(gold)
    print(f"{case} {kind}: device vs reference golden rel-L2 {rel:.3e}, bound {bound:.3e}; golden vs fp64 restatement "
          f"{float(gold[f'{case}__{kind}__ref_vs_fp64']):.3e}; captures, live replays {counters}")
    assert gammas == want
    assert torch.isfinite(y).all() and rel <= bound
    # the steps went through the whole-step graph, and it was rebuilt at every window edge
    assert not disabled and counters == C.expected_counters(want)[1:]


@pytest.mark.parametrize("case,kind", CASE_GUIDER, ids=IDS)
def test_analytic_cases_against_the_fp64_restatement(device_runs, gold, case, kind):
    from seva import sampling as S
    y, gammas, _, _ = device_runs(case, kind)
    st = C.settings(case, S.DDPMDiscretization())
    ref = C.restate_fp64(gold["noise"], gold[f"{case}__eps"], S.DDPMDiscretization()(st["steps"]), gammas, st["s_noise"],
                         C.frame_scale(kind, views_of(gold)))
    rel, bound = rel_l2(y, ref), bound_of(gold)
    print(f"{case} {kind}: device vs fp64 restatement (fp32 step scalars) rel-L2 {rel:.3e}, bound {bound:.3e}")
    assert rel <= bound


# ------------------------------------------------------------------ the tiny network
def _runner(net, dev, guider, steps, eps=None, cls=None, scene_seed=23, scale=2.0, **churn):
    """The SAME sampler, cond objects and denoiser callable serve every call of run() (`_runner` of
    tests/test_solver_dpmpp2m_gpu.py with the churn arguments)."""
    from seva import sampling as S
    from seva import synthetic as synth
    from seva.model import SGMWrapper
    sc = synth.synth_scene(T, (HW, HW), (0,), seed=scene_seed)
    disc = S.DDPMDiscretization()
    den = S.DiscreteDenoiser(disc, num_idx=1000, device=dev)
    sampler = (cls or S.EulerEDMSampler)(disc, guider, num_steps=steps, verbose=False, device=dev, **churn)
    wrap = SGMWrapper(net)
    cond = {k: v.to(dev) for k, v in sc["cond"].items()}
    uc = {k: v.to(dev) for k, v in sc["uc"].items()}
    kw = {} if not isinstance(guider, S.MultiviewCFG) else dict(
        c2w=sc["c2w"].to(dev), K=sc["K"].to(dev), input_frame_mask=sc["input_frame_mask"].to(dev))
    denoiser = lambda x, s, c: den(wrap, x, s, c, num_frames=T)  # noqa: E731

    def run(inference=False):
        if eps is not None:
            it = iter(eps)
            sampler.noise_fn = lambda x: next(it).to(x.device)
        if inference:
            with torch.inference_mode():
                return sampler(denoiser, sc["noise"].to(dev), scale=scale, cond=cond, uc=uc, verbose=False, **kw).clone()
        return sampler(denoiser, sc["noise"].to(dev), scale=scale, cond=cond, uc=uc, verbose=False, **kw)

    return run, sampler


def _counters(sampler):
    cache = sampler._step_graphs
    return cache.captures, (cache.graph.replays if cache.graph is not None else None)


def test_tiny_loop_against_the_reference_golden(dev, tiny, monkeypatch):
    """Six chained network calls with sigma_hat = sigma (1 + gamma) + 1e-6 in the nearest-sigma lookup and real noise between them."""
    from seva import sampling as S
    monkeypatch.delenv("SEVA_SOLVER", raising=False)
    net, _ = tiny
    g, t = load_golden(C.GOLDEN_TINY), C.TINY
    assert all(float(g[k]) == t[k] for k in t)
    assert torch.equal(g["eps"], torch.stack(C.eps_list(t["steps"], (T, 4, HW, HW), t["eps_seed"])))

    class Sampler(Recording, S.EulerEDMSampler):
        pass

    run, sm = _runner(net, dev, S.MultiviewCFG(C.CFG_MIN), t["steps"], list(g["eps"]), Sampler, t["scene_seed"], t["scale"],
                      s_churn=t["s_churn"], s_tmin=t["s_tmin"], s_tmax=t["s_tmax"], s_noise=t["s_noise"])
    y = run()
    want = [float(v) for v in g["gamma"]]
    err = rel_l2(y.cpu(), g["y"])
    print(f"tiny {t['steps']}-step loop, gamma {want}, vs reference golden: rel-L2 {err:.3e} (NET_TOL {NET_TOL:.0e}); "
          f"captures, live replays {_counters(sm)}")
    assert sm.gammas == want and _counters(sm) == C.expected_counters(want)[1:]
    assert err < NET_TOL


STEPS, S_NOISE, S_CHURN = 7, 1.003, 1.4  # gamma = 0.2 inside the window


def _windowed(dev):
    """Churn arguments whose window bounds are the schedule's own sigmas 2 and 4 -> gamma runs [0, 0, g, g, g, 0, 0]."""
    from seva import sampling as S
    sig = S.DDPMDiscretization()(STEPS)
    g = S_CHURN / STEPS
    return dict(s_churn=S_CHURN, s_tmin=float(sig[4]), s_tmax=float(sig[2]), s_noise=S_NOISE), [0.0, 0.0, g, g, g, 0.0, 0.0]


def _eps(seed=5):
    return C.eps_list(STEPS, (T, 4, HW, HW), seed)


@pytest.mark.parametrize("guider_kind", [0, 1, 2])
def test_whole_step_graph_equals_eager_across_window_edges(dev, tiny, guider_kind, monkeypatch):
    """Two key changes inside one trajectory: three warm-ups, three captures, and what each graph replays is the eager step, bit for
    bit -- also under torch.inference_mode(), and on a second trajectory on the same sampler and cond objects."""
    from seva import sampling as S
    net, _ = tiny
    churn, gammas = _windowed(dev)
    assert C.runs_of(gammas) == [2, 3, 2]
    mk = lambda: [S.VanillaCFG(), S.MultiviewCFG(1.2), S.MultiviewTemporalCFG(T, 1.2)][guider_kind]  # noqa: E731

    class Sampler(Recording, S.EulerEDMSampler):
        pass

    monkeypatch.delenv("SEVA_SOLVER", raising=False)
    monkeypatch.setenv("SEVA_STEPGRAPH", "0")
    monkeypatch.setenv("SEVA_HIPGRAPH", "0")
    run0, s0 = _runner(net, dev, mk(), STEPS, _eps(), Sampler, **churn)
    ref = run0()
    assert s0.gammas == gammas and _counters(s0) == (0, None) and torch.isfinite(ref).all()
    monkeypatch.setenv("SEVA_STEPGRAPH", "1")
    monkeypatch.setenv("SEVA_HIPGRAPH", "1")
    run1, s1 = _runner(net, dev, mk(), STEPS, _eps(), **churn)
    got = run1()
    print(f"guider {guider_kind}: gamma runs {C.runs_of(gammas)}: captures, live replays {_counters(s1)}")
    assert _counters(s1) == C.expected_counters(gammas)[1:] == (3, 1) and not s1._step_graphs.disabled
    assert torch.equal(got, ref)
    # one more trajectory, same sampler and cond objects: its first key is the last key of the first one (gamma 0 -> 0)
    again = run1()
    print(f"guider {guider_kind}: after a second trajectory {C.runs_of(gammas * 2)}: captures, live replays {_counters(s1)}")
    assert _counters(s1) == C.expected_counters(gammas * 2)[1:] == (5, 1)
    assert torch.equal(again, ref)
    run2, s2 = _runner(net, dev, mk(), STEPS, _eps(), **churn)
    got_i = run2(inference=True)
    assert _counters(s2) == (3, 1) and torch.equal(got_i, ref)
    # the churn reaches the result: another s_noise, other bits
    other, _ = _runner(net, dev, mk(), STEPS, _eps(), **dict(churn, s_noise=1.0))
    assert not torch.equal(other(), ref)


def test_default_noise_fn_graph_equals_eager(dev, tiny, monkeypatch):
    """`noise_fn` left at torch.randn_like, the device generator seeded before each run: nothing inside the captured step consumes
    the generator, and the eagerly drawn eps reaches the replay."""
    from seva import sampling as S
    net, _ = tiny
    churn, gammas = _windowed(dev)
    monkeypatch.delenv("SEVA_SOLVER", raising=False)
    monkeypatch.setenv("SEVA_STEPGRAPH", "0")
    monkeypatch.setenv("SEVA_HIPGRAPH", "0")
    run0, s0 = _runner(net, dev, S.MultiviewCFG(1.2), STEPS, None, **churn)
    assert s0.noise_fn is torch.randn_like
    torch.manual_seed(77)
    ref = run0()
    torch.manual_seed(78)
    assert not torch.equal(run0(), ref)  # the draw matters
    monkeypatch.setenv("SEVA_STEPGRAPH", "1")
    monkeypatch.setenv("SEVA_HIPGRAPH", "1")
    run1, s1 = _runner(net, dev, S.MultiviewCFG(1.2), STEPS, None, **churn)
    torch.manual_seed(77)
    got = run1()
    assert _counters(s0) == (0, None) and _counters(s1) == (3, 1)
    assert torch.equal(got, ref)


def test_tracked_sampler_computes_gamma_itself(dev, tiny, monkeypatch):
    """`test_tracked_sampler_subclass_protocol` of tests/test_model_gpu.py with s_churn > 0: the subclass compares `sigmas[i]` with
    the bounds and calls `sampler_step` with its own gamma; same bits as `EulerEDMSampler.__call__` on the same eps."""
    from seva import sampling as S
    net, _ = tiny
    churn, gammas = _windowed(dev)
    monkeypatch.delenv("SEVA_SOLVER", raising=False)

    class Tracked(S.EulerEDMSampler):
        steps_done = 0

        def __call__(self, denoiser, x, scale, cond, uc=None, num_steps=None, verbose=True, **guider_kwargs):
            uc = cond if uc is None else uc
            x, s_in, sigmas, num_sigmas, cond, uc = self.prepare_sampling_loop(x, cond, uc, num_steps)
            self.seen = []
            for i in self.get_sigma_gen(num_sigmas, verbose=verbose):
                gamma = min(self.s_churn / (num_sigmas - 1), 2 ** 0.5 - 1) if self.s_tmin <= sigmas[i] <= self.s_tmax else 0.0
                self.seen.append(gamma)
                x = self.sampler_step(s_in * sigmas[i], s_in * sigmas[i + 1], denoiser, x, scale, cond, uc, gamma, **guider_kwargs)
                self.steps_done += 1
            return x

    run0, s0 = _runner(net, dev, S.MultiviewCFG(1.2), STEPS, _eps(13), **churn)
    ref = run0(inference=True)
    run1, tracked = _runner(net, dev, S.MultiviewCFG(1.2), STEPS, _eps(13), Tracked, **churn)
    got = run1(inference=True)
    assert tracked.steps_done == STEPS and tracked.seen == gammas
    assert _counters(tracked) == _counters(s0) == (3, 1)
    assert torch.equal(got, ref)


def test_pinned_frame_moves_along_its_own_line_with_gamma(dev, tiny, monkeypatch):
    """The property `test_headline_sampler_step_finite_and_replayable` checks, with gamma > 0: the replace-blend pins the input
    frame, so one step moves it to x_noised + dt (x_noised - latent) / sigma_hat with x_noised = x + eps sqrt(sigma_hat^2 -
    sigma^2) s_noise.  fp64 on that frame from the fp32 step scalars; that test's bound."""
    from seva import sampling as S
    from seva import synthetic as synth
    from seva.model import SGMWrapper
    net, _ = tiny
    monkeypatch.delenv("SEVA_SOLVER", raising=False)
    sc = synth.synth_scene(T, (HW, HW), (0,), seed=23)
    disc = S.DDPMDiscretization()
    den = S.DiscreteDenoiser(disc, num_idx=1000, device=dev)
    gamma = 0.25
    sampler = S.EulerEDMSampler(disc, S.MultiviewCFG(1.2), num_steps=50, verbose=False, device=dev, s_churn=50 * gamma, s_noise=S_NOISE)
    eps = torch.randn(T, 4, HW, HW, generator=torch.Generator().manual_seed(1))
    sampler.noise_fn = lambda x: eps.to(x.device)
    wrap = SGMWrapper(net)
    cond = {k: v.to(dev) for k, v in sc["cond"].items()}
    uc = {k: v.to(dev) for k, v in sc["uc"].items()}
    gk = dict(c2w=sc["c2w"].to(dev), K=sc["K"].to(dev), input_frame_mask=sc["input_frame_mask"].to(dev))
    x, s_in, sigmas, n_sig, cond, uc = sampler.prepare_sampling_loop(sc["noise"].to(dev), cond, uc, None)
    f = lambda xx, ss, cc: den(wrap, xx, ss, cc, num_frames=T)  # noqa: E731
    x1 = sampler.sampler_step(s_in * sigmas[0], s_in * sigmas[1], f, x, 2.0, cond, uc, gamma, **gk)
    x2 = sampler.sampler_step(s_in * sigmas[0], s_in * sigmas[1], f, x, 2.0, cond, uc, gamma, **gk)
    assert torch.equal(x1, x2) and torch.isfinite(x1).all()  # eager warm-up, then the captured step
    assert _counters(sampler) == (1, 1)
    sigma_hat, nscale, dt = (v[0].double() for v in C.step_scalars(sigmas.cpu(), 0, gamma, T))
    assert float(nscale) > 0.7 * float(sigmas[0])  # the noise is no rounding artefact here
    lat = sc["cond"]["replace"][0:1, :4].double()
    x_noised = x[0:1].cpu().double() + eps[0:1].double() * nscale * S_NOISE
    expect = x_noised + dt * (x_noised - lat) / sigma_hat
    dev_err = float((x1[0:1].cpu().double() - expect).abs().max())
    print(f"pinned frame after one step with gamma {gamma}: max |x1 - closed form| {dev_err:.3e}, "
          f"bound 0.35 max|x1| = {0.35 * float(x1[0:1].abs().max()):.3e}")
    assert dev_err < 0.35 * float(x1[0:1].abs().max())
    # and without the noise term the closed form is far off: the check sees add_noise
    no_noise = x[0:1].cpu().double() + dt * (x[0:1].cpu().double() - lat) / sigma_hat
    assert float((x1[0:1].cpu().double() - no_noise).abs().max()) > 0.35 * float(x1[0:1].abs().max())
