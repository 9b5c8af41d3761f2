"""Opt-in guidance controls on the device: the `seva_cfg_rescale_f32` kernel against its contract (include/seva_hip.h) restated in
torch, its exact cases and its independence from the rest of the launch; and the sampler with `guidance_interval` /
`guidance_rescale` on the tiny synthetic network -- whole-step graphs against eager steps and against the loop over `seva.ops`
written out here, for both solvers, alone and with `cache_interval`.

Bounds of the kernel test (set by the contract, not by what the kernel returns): the reference takes g from `ops.cfg_combine` on
the device (the same device function), sums in torch fp64, rounds m to fp32 once and multiplies in fp32.  The kernel's fp64 sums
differ from torch's by summation order alone, ~1e-13 relative on inputs with |mean| <= std (which the test uses; N = 1 and constant
frames are the exact cases): that can move the single rounding of m by one fp32 ulp, and the multiply then adds one more.  Hence
|mult_out - m_ref| <= 1 ulp and |out - out_ref| <= 2 ulps of out_ref."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_model_gpu import dev, tiny  # noqa: E402,F401  (module-scoped fixtures, not copied into a conftest)

INF = float("inf")
SHAPES = [(1, 1), (1, 105), (3, 884), (5, 576), (2, 20736), (42, 324), (96, 576)]
PHIS = [0.0, 0.7, 1.0]
SCALES = (4.5, 0.0, 1.0, 2.0, 3.0)  # cycled over the frames: n = 1 gets 4.5, n >= 3 gets 0, 1 and 4.5


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def _case(n, chw):
    """(den2, scale, g32, S) on the device, computed once per shape and never written: |mean| <= std in every frame of both halves;
    g32 from `ops.cfg_combine`; S = the four fp64 sums (torch's order) as (n, 4)."""
    from seva import ops
    d = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1000 * n + chw % 997)
    u = 0.5 + torch.randn(n, chw, generator=g)
    c = -0.5 + 1.5 * torch.randn(n, chw, generator=g)
    den2 = torch.cat([u, c]).to(d)
    scale = torch.tensor([SCALES[i % len(SCALES)] for i in range(n)], device=d)
    g32 = torch.empty(n, chw, device=d)
    ops.cfg_combine(den2, scale, g32)
    cd, gd = den2[n:].double(), g32.double()
    S = torch.stack([cd.sum(1), (cd * cd).sum(1), gd.sum(1), (gd * gd).sum(1)], 1)
    return den2, scale, g32, S


def _m_ref(S, chw, phi):
    """m of the contract in fp64 from the sums (n, 4); phi as the float the ABI carries"""
    phi = _f32(phi)
    var_c = S[:, 1] - S[:, 0] * S[:, 0] / chw
    var_g = S[:, 3] - S[:, 2] * S[:, 2] / chw
    ok = (var_g > 0) & (var_c >= 0) & (phi > 0)
    safe = torch.where(ok, var_g, torch.ones_like(var_g))
    return torch.where(ok, phi * torch.sqrt(var_c / safe) + (1.0 - phi), torch.ones_like(var_g))


def _ulp(x):
    """spacing of fp32 at |x| (x fp32, normal range), as fp64"""
    _, e = torch.frexp(x)
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 24).clamp_min(2.0 ** -149)


@pytest.mark.parametrize("phi", PHIS)
@pytest.mark.parametrize("n,chw", SHAPES)
def test_kernel_against_the_contract(dev, n, chw, phi):
    from seva import ops
    den2, scale, g32, S = _case(n, chw)
    m_ref = _m_ref(S, chw, phi).float()
    out_ref = m_ref[:, None] * g32
    out, mult = torch.empty(n, chw, device=dev), torch.empty(n, device=dev)
    ops.cfg_rescale(den2, scale, phi, out, mult)
    dm = (mult.double() - m_ref.double()).abs() / _ulp(m_ref)
    do = (out.double() - out_ref.double()).abs() / _ulp(out_ref)
    mean_over_std = float((den2[n:].double().mean(1).abs() / den2[n:].double().std(1, correction=0).clamp_min(1e-300)).max()) if chw > 1 else 0.0
    print(f"\n(n, chw) = ({n}, {chw}) phi = {phi}: m in [{float(m_ref.min()):.6f}, {float(m_ref.max()):.6f}], "
          f"max |mult_out - m_ref| = {float(dm.max()):.1f} ulp, max |out - out_ref| = {float(do.max()):.1f} ulp, |mean|/std <= {mean_over_std:.2f}")
    assert torch.isfinite(out).all() and mean_over_std <= 1.0
    assert float(dm.max()) <= 1.0
    assert float(do.max()) <= 2.0
    if chw > 1 and phi > 0 and n >= 3:
        assert float(m_ref.min()) < 1.0 < float(m_ref.max())  # the multiplier is at work (scale 4.5 shrinks, scale 0 stretches)
    # mult_out is optional, and the result does not depend on it
    out2 = torch.empty_like(out)
    ops.cfg_rescale(den2, scale, phi, out2)
    assert torch.equal(out2, out)


@pytest.mark.parametrize("n,chw", SHAPES)
def test_phi_zero_is_cfg_combine_bit_for_bit(dev, n, chw):
    from seva import ops
    den2, scale, g32, _ = _case(n, chw)
    out, mult = torch.full((n, chw), -7.0, device=dev), torch.full((n,), -7.0, device=dev)
    ops.cfg_rescale(den2, scale, 0.0, out, mult)
    assert torch.equal(out, g32) and torch.equal(mult, torch.ones(n, device=dev))


@pytest.mark.parametrize("phi", [0.7, 1.0])
def test_exact_cases(dev, phi):
    """The select gives exactly 1: constant frames (values whose sums are exact in fp64), u == c with scale 1 (g IS c, so the two
    variances are the same number), one-element frames."""
    from seva import ops
    n, chw = 4, 1237
    g = torch.Generator().manual_seed(7)
    u = torch.randn(n, chw, generator=g)
    c = torch.randn(n, chw, generator=g)
    u[0], c[0] = 0.75, -1.5          # constant frame, guided value constant too
    u[1], c[1] = 2.0, 2.0            # constant and equal
    c[2] = u[2]                      # u == c, scale 1
    scale = torch.tensor([4.5, 2.0, 1.0, 3.0], device=dev)
    den2 = torch.cat([u, c]).to(dev)
    want = torch.empty(n, chw, device=dev)
    ops.cfg_combine(den2, scale, want)
    out, mult = torch.empty(n, chw, device=dev), torch.empty(n, device=dev)
    ops.cfg_rescale(den2, scale, phi, out, mult)
    assert torch.equal(mult[:3], torch.ones(3, device=dev)), mult
    assert torch.equal(out[:3], want[:3]) and mult[3] != 1.0
    one = torch.tensor([[0.3], [0.9], [-0.2], [0.4]], device=dev)  # n = 2, chw = 1
    o1, m1 = torch.empty(2, 1, device=dev), torch.empty(2, device=dev)
    ops.cfg_rescale(one, scale[:2].contiguous(), phi, o1, m1)
    w1 = torch.empty(2, 1, device=dev)
    ops.cfg_combine(one, scale[:2].contiguous(), w1)
    assert torch.equal(m1, torch.ones(2, device=dev)) and torch.equal(o1, w1)


def test_non_finite_inputs_propagate_through_g(dev):
    from seva import ops
    n, chw = 3, 300
    den2, scale, _, _ = _case(3, 884)
    den2 = den2[:, :chw].contiguous()
    den2[0, 5] = float("nan")       # uncond half of frame 0
    den2[n + 1, 7] = float("inf")   # cond half of frame 1
    want = torch.empty(n, chw, device=dev)
    ops.cfg_combine(den2, scale, want)
    out, mult = torch.empty(n, chw, device=dev), torch.empty(n, device=dev)
    ops.cfg_rescale(den2, scale, 0.7, out, mult)
    # the variances of frames 0 and 1 are NaN: the select leaves m = 1 and the non-finite values are g's own
    assert torch.equal(mult[:2], torch.ones(2, device=dev)) and torch.isfinite(mult[2])
    assert torch.equal(torch.isnan(out), torch.isnan(want)) and torch.equal(out[:2].nan_to_num(1.0, 2.0, 3.0), want[:2].nan_to_num(1.0, 2.0, 3.0))
    assert torch.isfinite(out[2]).all()


def test_a_frame_does_not_depend_on_its_surroundings(dev):
    from seva import ops
    n, chw, phi = 5, 576, 0.7
    den2, scale, _, _ = _case(n, chw)
    out, mult = torch.empty(n, chw, device=dev), torch.empty(n, device=dev)
    ops.cfg_rescale(den2, scale, phi, out, mult)
    again, mult2 = torch.empty_like(out), torch.empty_like(mult)
    ops.cfg_rescale(den2, scale, phi, again, mult2)
    assert torch.equal(again, out) and torch.equal(mult2, mult)  # two launches
    for k in range(n):  # frame k launched alone, and as the last frame of another batch
        alone = torch.cat([den2[k:k + 1], den2[n + k:n + k + 1]]).contiguous()
        o1, m1 = torch.empty(1, chw, device=dev), torch.empty(1, device=dev)
        ops.cfg_rescale(alone, scale[k:k + 1].contiguous(), phi, o1, m1)
        assert torch.equal(o1[0], out[k]) and m1[0] == mult[k], k
    order = [3, 0, 4]
    mixed = torch.cat([den2[order], den2[[n + i for i in order]]]).contiguous()
    o3, m3 = torch.empty(3, chw, device=dev), torch.empty(3, device=dev)
    ops.cfg_rescale(mixed, scale[order].contiguous(), phi, o3, m3)
    assert torch.equal(o3, out[order]) and torch.equal(m3, mult[order])


@pytest.mark.parametrize("n,chw", [(3, 884), (2, 105), (5, 576)])
def test_offset_pointers_and_guards(dev, n, chw):
    """Every base pointer one float off 16-byte alignment, and sentinels around `out` and `mult_out`."""
    from seva import ops
    phi, G, SENT = 0.7, 64, -12345.0
    den2, scale, _, _ = _case(n, chw)
    want, want_m = torch.empty(n, chw, device=dev), torch.empty(n, device=dev)
    ops.cfg_rescale(den2, scale, phi, want, want_m)

    def shifted(t):  # the same values at a base address that is 4 bytes past a 16-byte boundary
        buf = torch.empty(t.numel() + 1, device=dev)
        assert buf.data_ptr() % 16 == 0
        v = buf[1:].view(t.shape)
        v.copy_(t)
        return v

    obuf = torch.full((G + 1 + n * chw + G,), SENT, device=dev)
    mbuf = torch.full((G + 1 + n + G,), SENT, device=dev)
    out, mult = obuf[G + 1:G + 1 + n * chw].view(n, chw), mbuf[G + 1:G + 1 + n]
    d2, sc = shifted(den2), shifted(scale)
    assert all(t.data_ptr() % 16 == 4 and t.is_contiguous() for t in (d2, sc, out, mult))
    ops.cfg_rescale(d2, sc, phi, out, mult)
    assert torch.equal(out, want) and torch.equal(mult, want_m)
    for buf, size in ((obuf, n * chw), (mbuf, n)):
        assert bool((buf[:G + 1] == SENT).all()) and bool((buf[G + 1 + size:] == SENT).all())


def test_bad_arguments(dev):
    from seva import ops
    from seva._native import SevaNativeError
    n, chw = 3, 884
    den2, scale, _, _ = _case(n, chw)
    out, mult = torch.full((n, chw), 5.0, device=dev), torch.full((n,), 5.0, device=dev)
    for phi in (-0.1, 1.5, float("nan"), INF):
        with pytest.raises(SevaNativeError):
            ops.cfg_rescale(den2, scale, phi, out, mult)
    for args in ((den2[:-1], scale, 0.5, out, mult), (den2, scale[:-1], 0.5, out, mult), (den2, scale, 0.5, out, mult[:-1]),
                 (den2.half(), scale, 0.5, out, mult), (den2, scale, 0.5, out.t(), mult), (den2, scale.double(), 0.5, out, mult)):
        with pytest.raises(SevaNativeError):
            ops.cfg_rescale(*args)
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((mult == 5.0).all())  # a refused call launches nothing


# ------------------------------------------------------------------------------------------------ sampler, tiny network
T, HW, STEPS = 3, 8, 10   # the smallest latent the three-level network accepts
INTERVAL, PHI = (3.0, 25.0), 0.7  # guides steps 3..7 of the 10-step schedule (sigmas 84.9 48.3 30.0 19.8 13.5 9.35 6.34 4.05 2.26 0.90)
GUIDED = [False, False, False, True, True, True, True, True, False, False]
ENV = ("SEVA_SOLVER", "SEVA_CACHE_INTERVAL", "SEVA_CACHE_LEVELS", "SEVA_GUIDANCE_INTERVAL", "SEVA_GUIDANCE_RESCALE")


def _scene(dev):
    from seva import sampling as S
    from seva import synthetic as synth
    sc = synth.synth_scene(T, (HW, HW), (0,), seed=23)
    cond = {k: v.to(dev) for k, v in sc["cond"].items()}
    uc = {k: v.to(dev) for k, v in sc["uc"].items()}
    kw = dict(c2w=sc["c2w"].to(dev), K=sc["K"].to(dev), input_frame_mask=sc["input_frame_mask"].to(dev))
    disc = S.DDPMDiscretization()
    return sc["noise"], cond, uc, kw, disc, S.DiscreteDenoiser(disc, num_idx=1000, device=dev)


def _eps():
    g = torch.Generator().manual_seed(5)
    return [torch.randn(T, 4, HW, HW, generator=g) for _ in range(STEPS)]


def _runner(net, dev, solver, **kw_sampler):
    """The same sampler, cond objects and denoiser callable for every call of run()"""
    from seva import sampling as S
    from seva.model import SGMWrapper
    noise, cond, uc, kw, disc, den = _scene(dev)
    sampler = S.EulerEDMSampler(disc, S.MultiviewCFG(1.2), num_steps=STEPS, verbose=False, device=dev, s_churn=0.0, solver=solver,
                                **kw_sampler)
    wrap = SGMWrapper(net)
    denoiser = lambda x, s, c: den(wrap, x, s, c, num_frames=T)  # noqa: E731
    eps = _eps()

    def run():
        it = iter(eps)
        sampler.noise_fn = lambda x: next(it).to(x.device)
        return sampler(denoiser, noise.to(dev), scale=2.0, cond=cond, uc=uc, verbose=False, **kw)

    return run, sampler


def _written_out(net, dev, solver, interval, phi):
    """The trajectory as a plain loop over `seva.ops`: per step the denoiser on the CFG batch or on the conditional inputs alone,
    `ops.cfg_rescale` where the step is guided, and the plain update of the solver."""
    from seva import ops
    from seva import sampling as S
    from seva.model import SGMWrapper
    noise, cond, uc, kw, disc, den = _scene(dev)
    guider, wrap, eps = S.MultiviewCFG(1.2), SGMWrapper(net), _eps()
    network = lambda xin, t, c: wrap(xin, t, c, num_frames=T)  # noqa: E731
    sigmas = disc(STEPS, device=dev)
    host = sigmas.cpu()
    x = noise.to(dev).clone()
    s_in = x.new_ones([T])
    ops.scale_rows(x, torch.sqrt(1.0 + sigmas[0] ** 2.0).expand(T).contiguous(), x)
    hist, prev = torch.zeros_like(x), torch.zeros_like(s_in)
    flags = []
    for i in range(STEPS):
        sigma, nxt = s_in * sigmas[i], s_in * sigmas[i + 1]
        out = torch.empty_like(x)
        if solver == "euler":
            sigma_in = sigma * (0.0 + 1.0) + 1e-6
            x_in = torch.empty_like(x)
            ops.add_noise(x, eps[i].to(dev), ((sigma_in**2 - sigma**2) ** 0.5 * 1.0).contiguous(), x_in)
        else:
            sigma_in, x_in = sigma, x
        guided = bool(interval[0] < host[i] <= interval[1])
        flags.append(guided)
        if guided:
            den2 = den(network, *guider.prepare_inputs(x_in, sigma_in, cond, uc))
            fs = S._scale_vector(guider.frame_scale(den2, sigma_in, 2.0, **kw), T, x.device)
            D = torch.empty_like(x)
            ops.cfg_rescale(den2, fs, phi, D)
        else:
            D = den(network, x_in, sigma_in, dict(cond))
        if solver == "euler":
            ops.euler_step(x_in, D, sigma_in, nxt - sigma_in, out)
        else:
            a, b, c = S.EulerEDMSampler.multistep_coefficients(sigma, nxt, prev)
            ops.cfg_multistep(x, D, None, hist, a, b, c, out, hist)
            prev = sigma
        x = out
    assert flags == GUIDED
    return x


@pytest.fixture
def clean_env(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


@pytest.mark.parametrize("solver", ["euler", "dpmpp2m"])
def test_sampler_graph_is_eager_is_the_loop_written_out(dev, tiny, solver, clean_env):
    net, _ = tiny
    want = _written_out(net, dev, solver, INTERVAL, PHI)
    assert torch.isfinite(want).all()
    clean_env.setenv("SEVA_STEPGRAPH", "0")
    run0, s0 = _runner(net, dev, solver, guidance_interval=INTERVAL, guidance_rescale=PHI)
    got0 = run0()
    assert s0._step_graphs.captures == 0 and torch.equal(got0, want)
    clean_env.setenv("SEVA_STEPGRAPH", "1")
    run1, s1 = _runner(net, dev, solver, guidance_interval=INTERVAL, guidance_rescale=PHI)
    got1 = run1()
    cache = s1._step_graphs
    U = (0, "unguided")
    # unguided steps 0 1 2 8 9: warm-up, capture + replay, 3 replays; guided steps 3..7: warm-up, capture + replay, 3 replays
    assert torch.equal(got1, want) and not cache.disabled and cache.captures == 2 and set(cache.entries) == {0, U}
    assert (cache.entries[U].graph.replays, cache.entries[0].graph.replays) == (4, 4)
    # a second trajectory through the same sampler: both graphs serve it from the first step on
    assert torch.equal(run1(), want)
    assert cache.captures == 2 and (cache.entries[U].graph.replays, cache.entries[0].graph.replays) == (4 + 5, 4 + 5)
    # each control changes the result (the test would pass on a sampler that ignored them otherwise)
    plain = _runner(net, dev, solver)[0]()
    only_interval = _runner(net, dev, solver, guidance_interval=INTERVAL)[0]()
    assert not torch.equal(plain, want) and not torch.equal(only_interval, want) and not torch.equal(only_interval, plain)


@pytest.mark.parametrize("solver", ["euler", "dpmpp2m"])
def test_the_whole_interval_with_phi_zero_is_the_sampler_as_it_was(dev, tiny, solver, clean_env):
    net, _ = tiny
    off, s_off = _runner(net, dev, solver)
    on, s_on = _runner(net, dev, solver, guidance_interval=(0, INF), guidance_rescale=0)
    a, b = off(), on()
    assert torch.equal(a, b) and torch.isfinite(a).all()
    assert set(s_on._step_graphs.entries) == {0} and s_on._step_graphs.captures == s_off._step_graphs.captures == 1


@pytest.mark.parametrize("solver", ["euler", "dpmpp2m"])
def test_with_cache_interval(dev, tiny, solver, clean_env):
    """F S S F S S F S F F: the step after each boundary is full, so no shallow call meets a full call of another batch (the
    engine would refuse it with a "signature" error), and the four step kinds replay from graphs of their own."""
    net, _ = tiny
    kw = dict(guidance_interval=INTERVAL, guidance_rescale=PHI, cache_interval=3, cache_levels=1)
    clean_env.setenv("SEVA_STEPGRAPH", "0")
    eager = _runner(net, dev, solver, **kw)[0]()
    clean_env.setenv("SEVA_STEPGRAPH", "1")
    run, sm = _runner(net, dev, solver, **kw)
    got = run()
    cache = sm._step_graphs
    assert torch.isfinite(got).all() and torch.equal(got, eager) and not cache.disabled
    assert set(cache.entries) == {0, 1, (0, "unguided"), (1, "unguided")} and cache.captures == 4
    assert torch.equal(run(), eager)
    assert not torch.equal(_runner(net, dev, solver, guidance_interval=INTERVAL, guidance_rescale=PHI)[0](), eager)


def test_audit_sees_cfg_rescale(dev, tiny, clean_env):
    from seva import audit
    net, _ = tiny
    run, _ = _runner(net, dev, "euler", guidance_interval=INTERVAL, guidance_rescale=PHI)
    with audit.record() as rec:
        out = run()
    rows = [r for r in rec.report().rows if r.op == "cfg_rescale"]
    assert torch.isfinite(out).all() and len(rows) == sum(GUIDED)
    assert all(r.output == "out" and r.rows * r.cols == T * 4 * HW * HW and r.inf + r.nan == 0 for r in rows)
