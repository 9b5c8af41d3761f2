"""Opt-in DPM-Solver++(2M) solver of `seva.sampling` (solver="dpmpp2m"), host logic: coefficients, order of accuracy,
history ownership, interface.  The HIP operators are emulated the way tests/test_pipeline_cpu.py does it (tests/fake_ops.py);
the new operator `ops.cfg_multistep` is emulated in this file in fp32 torch.  The fp64 restatement of the solver (sgm's
DPMPP2MSampler form, mult1..4 from t = -ln sigma) lives here too."""
import math

import pytest
import torch

from test_pipeline_cpu import _fake_net, _patch_cpu, _scene

S2, MU_U, MU_C, SCALE = 1.0, 0.3, -0.2, 2.0  # analytic CFG denoiser: data N(mu, s^2) with s = 1
MU = MU_U + SCALE * (MU_C - MU_U)
SHAPE = (4, 4, 6, 5)


def _rows(v, x):
    return v.view(-1, *([1] * (x.ndim - 1)))


def _fake_cfg_multistep(x, den, scale, old_den, a, b, c, out, den_out=None):
    """fp32 emulation of seva_cfg_multistep_f32 (every index read before it is written; c == 0 selects)."""
    if scale is not None:
        u, cd = den.chunk(2)
        d = u + _rows(scale, u) * (cd - u)
    else:
        d = den.clone()
    r = _rows(a, x) * x + _rows(b, x) * d
    if old_den is not None:
        r = torch.where(_rows(c, x) != 0, r + _rows(c, x) * old_den, r)
    if den_out is not None:
        den_out.copy_(d)
    out.copy_(r)


@pytest.fixture
def cpu_ops(monkeypatch):
    """fake_ops installed + the emulated new operator behind a spy; yields the list of recorded calls."""
    import seva.ops as ops
    monkeypatch.delenv("SEVA_SOLVER", raising=False)
    _patch_cpu(monkeypatch)
    calls = []

    def spy(x, den, scale, old_den, a, b, c, out, den_out=None):
        calls.append(dict(a=a.clone(), b=b.clone(), c=c.clone(), old_is_out=old_den is den_out, scaled=scale is not None))
        _fake_cfg_multistep(x, den, scale, old_den, a, b, c, out, den_out)

    monkeypatch.setattr(ops, "cfg_multistep", spy, raising=False)
    return calls


def _denoiser(xx, ss, cc):
    """[uncond ; cond] halves of the analytic denoiser D = mu (1 - k) + x k, k = s^2 / (s^2 + sigma^2)."""
    n = xx.shape[0] // 2
    k = _rows(S2 / (S2 + ss * ss), xx)
    mu = torch.cat([torch.full((n,), MU_U), torch.full((n,), MU_C)]).to(xx.dtype).view(-1, 1, 1, 1)
    return mu * (1 - k) + xx * k


def _noise(seed=11):
    return torch.randn(SHAPE, generator=torch.Generator().manual_seed(seed))


def _sampler(solver, steps=None, cls=None, **kw):
    from seva import sampling as S
    sm = (cls or S.EulerEDMSampler)(S.DDPMDiscretization(), S.VanillaCFG(), num_steps=steps, verbose=False, device="cpu",
                                    solver=solver, **kw)
    sm.noise_fn = torch.zeros_like  # the Euler step's 1e-6 sigma_hat offset would inject sqrt(2e-6 sigma) of noise: keep it an ODE solver
    return sm


def _solve(solver, steps, noise=None, sampler=None):
    sm = sampler or _sampler(solver, steps)
    x = (_noise() if noise is None else noise).clone()
    return sm(_denoiser, x, SCALE, {}, {}, num_steps=steps, verbose=False)


def _exact(noise):
    from seva import sampling as S
    s0 = float(S.DDPMDiscretization()(25)[0])  # sigma_0 is the same for every step count below 1000
    x0 = noise.double() * math.sqrt(1.0 + s0 * s0)
    return MU + (x0 - MU) * math.sqrt(S2 / (S2 + s0 * s0))


def _err(x, ref):
    return float((x.double() - ref).norm() / ref.norm())


def _sgm_coefficients(sigmas64):
    """sgm's DPMPP2MSampler: h = t+ - t, r = h_last / h, mult1 = s+/s, mult2 = expm1(-h), mult3 = 1 + 1/(2r), mult4 = 1/(2r);
    x+ = mult1 x - mult2 (mult3 D - mult4 D-), first order (x+ = mult1 x - mult2 D) on the first step and where s+ = 0.
    Returned as (a, b, c) of x+ = a x + b D + c D-, fp64."""
    out = []
    for i in range(len(sigmas64) - 1):
        s, sn = sigmas64[i], sigmas64[i + 1]
        mult1 = sn / s
        if sn == 0:
            out.append((0.0, 1.0, 0.0))
            continue
        h = -math.log(sn) + math.log(s)
        mult2 = math.expm1(-h)
        if i == 0:
            out.append((mult1, -mult2, 0.0))
            continue
        r = (-math.log(s) + math.log(sigmas64[i - 1])) / h
        out.append((mult1, -mult2 * (1 + 1 / (2 * r)), mult2 / (2 * r)))
    return out


@pytest.mark.parametrize("steps", [8, 25, 50])
def test_coefficients_equal_the_sgm_form(cpu_ops, steps):
    from seva import sampling as S
    _solve("dpmpp2m", steps)
    assert len(cpu_ops) == steps and all(c["old_is_out"] and c["scaled"] for c in cpu_ops)
    sig = [float(v) for v in S.DDPMDiscretization()(steps).double()]
    ref = _sgm_coefficients(sig)
    for i, (call, (a, b, c)) in enumerate(zip(cpu_ops, ref)):
        for name, want in (("a", a), ("b", b), ("c", c)):
            got = call[name].double()
            assert got.shape == (SHAPE[0],) and call[name].dtype == torch.float32
            assert float((got - want).abs().max()) <= 1e-5 * abs(want), (steps, i, name, got, want)
    first, last = cpu_ops[0], cpu_ops[-1]
    assert torch.equal(first["c"], torch.zeros(SHAPE[0])) and torch.equal(first["b"], 1.0 - first["a"])
    for name, want in (("a", 0.0), ("b", 1.0), ("c", 0.0)):
        assert torch.equal(last[name], torch.full((SHAPE[0],), want))
    assert all(float(c["c"].abs().min()) > 0 for c in cpu_ops[1:-1])  # every step in between is second order


def test_second_order_beats_euler_at_half_and_quarter_the_steps(cpu_ops):
    """Fails on any first-order implementation: Euler's error halves with the step count, so 25 first-order steps cannot
    beat 50 Euler steps.  fp64 values: 2.39e-2 < 6.2e-2 and 4.8e-3 < 3.2e-2; the fp32 rounding of the loop is ~2e-7."""
    noise = _noise()
    ref = _exact(noise)
    e = {(s, n): _err(_solve(s, n, noise), ref) for s, n in (("dpmpp2m", 25), ("euler", 50), ("dpmpp2m", 50), ("euler", 100))}
    print({k: f"{v:.3e}" for k, v in e.items()})
    assert e["dpmpp2m", 25] < e["euler", 50]
    assert e["dpmpp2m", 50] < e["euler", 100]


def test_degenerate_lengths(cpu_ops):
    from seva import sampling as S
    noise = _noise()
    s0 = S.DDPMDiscretization()(1)[0]
    x0 = noise * torch.sqrt(1.0 + s0 ** 2.0)
    u, c = _denoiser(torch.cat([x0, x0]), (torch.ones(2 * SHAPE[0]) * s0), {}).chunk(2)
    assert torch.equal(_solve("dpmpp2m", 1, noise), u + SCALE * (c - u))  # one step: sigma+ = 0, the denoiser's output at sigma_0
    del cpu_ops[:]
    _solve("dpmpp2m", 2, noise)
    assert len(cpu_ops) == 2 and all(torch.equal(c["c"], torch.zeros(SHAPE[0])) for c in cpu_ops)


def _partial(sampler, noise, steps, stop_after):
    x, s_in, sigmas, num_sigmas, cond, uc = sampler.prepare_sampling_loop(noise.clone(), {}, {}, steps)
    for i in range(stop_after):
        x = sampler.sampler_step(s_in * sigmas[i], s_in * sigmas[i + 1], _denoiser, x, SCALE, cond, uc, 0.0)
    return x


def test_history_belongs_to_one_trajectory(cpu_ops):
    n1, n2 = _noise(1), _noise(2)
    fresh1, fresh2 = _solve("dpmpp2m", 6, n1), _solve("dpmpp2m", 6, n2)
    assert not torch.equal(fresh1, fresh2)
    sm = _sampler("dpmpp2m", 6)
    assert torch.equal(_solve("dpmpp2m", 6, n1, sm), fresh1)
    assert torch.equal(_solve("dpmpp2m", 6, n2, sm), fresh2)
    # a trajectory stopped after 3 of 6 steps leaves its history behind; the next one must not see it (NaN included)
    sm = _sampler("dpmpp2m", 6)
    _partial(sm, n1, 6, 3)
    assert sm._ms_have
    assert torch.equal(_solve("dpmpp2m", 6, n2, sm), fresh2)
    _partial(sm, n1, 6, 3)
    sm._ms_den.fill_(float("nan"))
    assert torch.equal(_solve("dpmpp2m", 6, n2, sm), fresh2)


def test_tracked_style_subclass_gives_the_same_bits(cpu_ops):
    from seva import sampling as S

    class Tracked(S.EulerEDMSampler):  # drives the loop itself, like the reference's GradioTrackedSampler
        def __call__(self, denoiser, x, scale, cond, uc=None, num_steps=None, verbose=True, **guider_kwargs):
            uc = cond if uc is None else uc
            x, s_in, sigmas, num_sigmas, cond, uc = self.prepare_sampling_loop(x, cond, uc, num_steps)
            for i in self.get_sigma_gen(num_sigmas, verbose=verbose):
                gamma = min(self.s_churn / (num_sigmas - 1), 2 ** 0.5 - 1) if self.s_tmin <= sigmas[i] <= self.s_tmax else 0.0
                x = self.sampler_step(s_in * sigmas[i], s_in * sigmas[i + 1], denoiser, x, scale, cond, uc, gamma, **guider_kwargs)
                assert isinstance(x, torch.Tensor)  # sampler_step still returns x alone
            return x

    noise = _noise(3)
    tracked = _sampler("dpmpp2m", 7, cls=Tracked)
    assert torch.equal(_solve("dpmpp2m", 7, noise, tracked), _solve("dpmpp2m", 7, noise))


def test_guider_without_frame_scale_takes_the_combined_form(cpu_ops):
    from seva import sampling as S

    class PlainGuider:
        def prepare_inputs(self, x, s, c, uc):
            return S.VanillaCFG().prepare_inputs(x, s, c, uc)

        def __call__(self, x, sigma, scale):
            u, c = x.chunk(2)
            return u + scale * (c - u)

    noise = _noise(4)
    sm = _sampler("dpmpp2m", 5)
    sm.guider = PlainGuider()
    got = _solve("dpmpp2m", 5, noise, sm)
    assert not any(c["scaled"] for c in cpu_ops)
    assert torch.equal(got, _solve("dpmpp2m", 5, noise))


def test_solver_selection(cpu_ops, monkeypatch):
    from seva import sampling as S
    mk = lambda **kw: S.EulerEDMSampler(S.DDPMDiscretization(), S.VanillaCFG(), num_steps=3, device="cpu", **kw)  # noqa: E731
    assert mk().solver == "euler"
    monkeypatch.setenv("SEVA_SOLVER", "dpmpp2m")
    assert mk().solver == "dpmpp2m" and mk(solver="euler").solver == "euler"
    monkeypatch.setenv("SEVA_SOLVER", "heun")
    with pytest.raises(ValueError):
        mk()
    monkeypatch.delenv("SEVA_SOLVER")
    with pytest.raises(ValueError):
        mk(solver="dpmpp3m")
    with pytest.raises(ValueError):
        mk(solver="dpmpp2m", s_churn=0.5)
    assert mk(solver="euler", s_churn=0.5).solver == "euler"
    d = S.DPMPP2MSampler(S.DDPMDiscretization(), S.VanillaCFG(), num_steps=3, device="cpu")
    assert isinstance(d, S.EulerEDMSampler) and d.solver == "dpmpp2m"
    with pytest.raises(ValueError):
        S.DPMPP2MSampler(S.DDPMDiscretization(), S.VanillaCFG(), num_steps=3, device="cpu", s_churn=1.0)


@pytest.mark.parametrize("how", ["argument", "environment"])
def test_pipeline_passes_the_solver_to_the_sampler(cpu_ops, monkeypatch, how):
    from seva import pipeline
    from seva import sampling as S
    seen = []
    c2ws, Ks, lat, tok = _scene(43)
    kw = {}
    if how == "argument":
        kw["solver"] = "dpmpp2m"
    else:
        monkeypatch.setenv("SEVA_SOLVER", "dpmpp2m")
    res = pipeline.run_trajectory(_fake_net, lat, c2ws, Ks, [0], clip_token=tok, T=21, num_steps=3, seed=23, device="cpu",
                                  sampler_hook=lambda sm: seen.append(sm), **kw)
    assert seen and all(isinstance(sm, S.EulerEDMSampler) and sm.solver == "dpmpp2m" for sm in seen)
    assert len(cpu_ops) == 3 * len(seen) and torch.isfinite(res["latents"]).all()
    # and an explicit "euler" beats the variable all the way down
    del seen[:], cpu_ops[:]
    pipeline.run_trajectory(_fake_net, lat, c2ws, Ks, [0], clip_token=tok, T=21, num_steps=3, seed=23, device="cpu",
                            sampler_hook=lambda sm: seen.append(sm), solver="euler")
    assert seen and all(sm.solver == "euler" for sm in seen) and not cpu_ops


def test_default_path_is_untouched_and_multistep_draws_no_noise(cpu_ops, monkeypatch):
    import seva.ops as ops
    draws, noised = [], []

    def noise_fn(x):
        draws.append(1)
        return torch.zeros_like(x)

    real_add_noise = ops.add_noise
    monkeypatch.setattr(ops, "add_noise", lambda *a: (noised.append(1), real_add_noise(*a))[1])
    for solver in ("euler", None):
        del draws[:], noised[:], cpu_ops[:]
        sm = _sampler(solver, 5)
        assert sm.solver == "euler"
        sm.noise_fn = noise_fn
        _solve("euler", 5, sampler=sm)
        assert len(draws) == 5 and len(noised) == 5 and not cpu_ops
    del draws[:], noised[:]
    sm = _sampler("dpmpp2m", 5)
    sm.noise_fn = noise_fn
    _solve("dpmpp2m", 5, sampler=sm)
    assert not draws and not noised and len(cpu_ops) == 5
