"""`seva_cfg_multistep_f32` and the solver="dpmpp2m" sampler on the device: the kernel against fp64 with derived bounds,
aliasing, guard regions, batch invariance, loud errors; the sampler against its fp64 restatement on an analytic denoiser;
the whole-step hipGraph (graph == eager bitwise, history across trajectories); the default solver untouched."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_model_gpu import _loop, dev, tiny  # noqa: E402,F401  (module-scoped fixtures, not copied into a conftest)

U = 2.0 ** -24  # one fp32 rounding, relative
SHAPES = [(4, 3, 5, 7), (1, 4, 1, 1), (5, 4, 331, 331)]  # chw = 105 (odd); one element per image; > 8192 x 256 elements


def _col(v):
    return v.double().view(-1, 1, 1, 1)


def _case(shape, scaled, dev, seed=0):
    """Inputs with per-image coefficients all different; row 1 (where there is one) is the last step's (0, 1, 0); the row
    before the last has c = 0 and a history slice full of NaN."""
    g = torch.Generator().manual_seed(100 + seed)
    n = shape[0]
    r = lambda lead=n, s=1.0: (torch.randn((lead,) + shape[1:], generator=g) * s).to(dev)  # noqa: E731
    x, den, old = r(s=10.0), r(2 * n if scaled else n), r()
    a = torch.linspace(0.55, 0.95, n) if n > 1 else torch.tensor([0.7])
    b = (1 - a) * torch.linspace(1.3, 1.9, n)[:n]
    c = -(1 - a) * torch.linspace(0.3, 0.9, n)[:n]
    if n > 1:
        a[1], b[1], c[1] = 0.0, 1.0, 0.0
    nan_row = n - 2 if n > 2 else 0
    c[nan_row] = 0.0
    old[nan_row] = float("nan")
    scale = torch.linspace(1.2, 2.0, n).to(dev) if scaled else None
    return dict(x=x, den=den, old=old, a=a.to(dev), b=b.to(dev), c=c.to(dev), scale=scale, nan_row=nan_row)


def _ref(i):
    """-> (out, D, bound on |out - ref|, bound on |den_out - D|) in fp64 from the fp32 inputs."""
    n = i["x"].shape[0]
    x = i["x"].double()
    if i["scale"] is not None:
        u, cd, s = i["den"][:n].double(), i["den"][n:].double(), _col(i["scale"])
        D = u + s * (cd - u)
        magD = u.abs() + s.abs() * (cd.abs() + u.abs())
    else:
        D = i["den"].double()
        magD = D.abs()
    a, b, c = _col(i["a"]), _col(i["b"]), _col(i["c"])
    old = torch.where(c != 0, i["old"].double(), torch.zeros_like(x))  # c == 0: the two-term formula, whatever the history holds
    out = a * x + b * D + c * old
    return out, D, 8 * U * (a.abs() * x.abs() + b.abs() * magD + c.abs() * old.abs()), 4 * U * magD


@pytest.mark.parametrize("with_den_out", [True, False])
@pytest.mark.parametrize("scaled", [True, False])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_fp64(dev, shape, scaled, with_den_out):
    from seva import ops
    i = _case(shape, scaled, dev)
    out = torch.full(shape, float("nan"), device=dev)
    den_out = torch.full(shape, float("nan"), device=dev) if with_den_out else None
    ops.cfg_multistep(i["x"], i["den"], i["scale"], i["old"], i["a"], i["b"], i["c"], out, den_out)
    ref, D, bound, dbound = _ref(i)
    assert torch.isfinite(out).all()
    err = (out.double() - ref).abs()
    print(f"max |out - ref| / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    if with_den_out:
        assert torch.isfinite(den_out).all()
        derr = (den_out.double() - D).abs()
        print(f"max |den_out - D| / bound = {float((derr / dbound.clamp_min(1e-300)).max()):.3f}")
        assert bool((derr <= dbound).all())
        if not scaled:
            assert torch.equal(den_out, i["den"])
    if shape[0] > 1 and (with_den_out or not scaled):  # the (0, 1, 0) row returns D itself: 0 * x + 1 * D is exact
        assert torch.equal(out[1], den_out[1] if with_den_out else i["den"][1])


def test_no_history_pointer_means_no_history_term(dev):
    from seva import ops
    i = _case(SHAPES[0], True, dev)
    zero = torch.zeros_like(i["c"])
    got, want = torch.empty_like(i["x"]), torch.empty_like(i["x"])
    ops.cfg_multistep(i["x"], i["den"], i["scale"], None, i["a"], i["b"], zero, got)
    ops.cfg_multistep(i["x"], i["den"], i["scale"], torch.full_like(i["x"], float("nan")), i["a"], i["b"], zero, want)
    assert torch.isfinite(got).all() and torch.equal(got, want)


@pytest.mark.parametrize("scaled", [True, False])
def test_aliasing_gives_the_same_bits(dev, scaled):
    from seva import ops
    i = _case(SHAPES[0], scaled, dev)
    out, den_out = torch.empty_like(i["x"]), torch.empty_like(i["x"])
    ops.cfg_multistep(i["x"], i["den"], i["scale"], i["old"], i["a"], i["b"], i["c"], out, den_out)
    x, hist = i["x"].clone(), i["old"].clone()
    ops.cfg_multistep(x, i["den"], i["scale"], hist, i["a"], i["b"], i["c"], x, hist)  # out is x, den_out is old_den
    assert torch.equal(x, out) and torch.equal(hist, den_out)


@pytest.mark.parametrize("shape", SHAPES[:2] + [(2, 4, 331, 331)], ids=lambda s: "x".join(map(str, s)))
def test_guard_regions_stay_untouched(dev, shape):
    from seva import ops
    i = _case(shape, True, dev)
    count, pad, sentinel = math.prod(shape), 1031, -1234.5
    bufs = [torch.full((count + 2 * pad,), sentinel, device=dev) for _ in range(2)]
    out, den_out = (b[pad:pad + count].view(shape) for b in bufs)
    ops.cfg_multistep(i["x"], i["den"], i["scale"], i["old"], i["a"], i["b"], i["c"], out, den_out)
    want_out, want_den = torch.empty_like(i["x"]), torch.empty_like(i["x"])
    ops.cfg_multistep(i["x"], i["den"], i["scale"], i["old"], i["a"], i["b"], i["c"], want_out, want_den)
    for b, want in zip(bufs, (want_out, want_den)):
        assert bool((b[:pad] == sentinel).all()) and bool((b[pad + count:] == sentinel).all())
        assert torch.equal(b[pad:pad + count].view(shape), want)


@pytest.mark.parametrize("scaled", [True, False])
def test_rows_do_not_depend_on_the_batch(dev, scaled):
    from seva import ops
    shape = (5, 3, 5, 7)
    i = _case(shape, scaled, dev)
    out, den_out = torch.empty_like(i["x"]), torch.empty_like(i["x"])
    ops.cfg_multistep(i["x"], i["den"], i["scale"], i["old"], i["a"], i["b"], i["c"], out, den_out)
    n = shape[0]
    for r in range(n):
        sl = slice(r, r + 1)
        den = torch.cat([i["den"][sl], i["den"][n + r:n + r + 1]]) if scaled else i["den"][sl]
        o1, d1 = torch.empty_like(i["x"][sl]), torch.empty_like(i["x"][sl])
        ops.cfg_multistep(i["x"][sl].contiguous(), den.contiguous(), i["scale"][sl].contiguous() if scaled else None,
                          i["old"][sl].contiguous(), i["a"][sl].contiguous(), i["b"][sl].contiguous(),
                          i["c"][sl].contiguous(), o1, d1)
        assert torch.equal(o1, out[sl]) and torch.equal(d1, den_out[sl]), r


def test_errors_are_loud(dev):
    from seva import ops
    from seva._native import SevaNativeError
    i = _case(SHAPES[0], True, dev)
    out = torch.empty_like(i["x"])
    args = lambda **kw: [kw.get(k, i[k]) for k in ("x", "den", "scale", "old", "a", "b", "c")]  # noqa: E731
    with pytest.raises(SevaNativeError):
        ops.cfg_multistep(*args(x=i["x"].cpu()), out)
    with pytest.raises(SevaNativeError):
        ops.cfg_multistep(*args(), out.cpu())
    with pytest.raises(SevaNativeError):  # n = 0
        e = torch.empty((0, 3, 5, 7), device=dev)
        v = torch.empty((0,), device=dev)
        ops.cfg_multistep(e, e, v, e, v, v, v, e.clone())
    with pytest.raises(SevaNativeError):  # [n][chw] den with a scale vector (needs [2n][chw])
        ops.cfg_multistep(*args(den=i["den"][:4].contiguous()), out)
    with pytest.raises(SevaNativeError):
        ops.cfg_multistep(*args(a=i["a"][:3].contiguous()), out)
    with pytest.raises(SevaNativeError):
        ops.cfg_multistep(*args(old=i["old"][:, :2].contiguous()), out)
    with pytest.raises(SevaNativeError):
        ops.cfg_multistep(*args(), out, torch.empty((4, 3, 5, 8), device=dev))
    with pytest.raises(SevaNativeError):
        ops.cfg_multistep(*args(), out.double())


# ------------------------------------------------------------------ the sampler on an analytic denoiser
S2, MU_U, MU_C, SCALE = 1.0, 0.3, -0.2, 2.0
MU = MU_U + SCALE * (MU_C - MU_U)
XSHAPE = (4, 4, 6, 5)


def _analytic(dev, dtype=torch.float32):
    n = XSHAPE[0]
    mu = torch.cat([torch.full((n,), MU_U), torch.full((n,), MU_C)]).to(device=dev, dtype=dtype).view(-1, 1, 1, 1)

    def denoiser(xx, ss, cc):
        k = (S2 / (S2 + ss * ss)).view(-1, 1, 1, 1)
        return mu * (1 - k) + xx * k

    return denoiser


def _dpmpp2m_fp64(noise, sigmas):
    """The solver restated in fp64 (sgm's DPMPP2MSampler on the guided analytic denoiser), from the fp32 sigmas."""
    sig = [float(v) for v in sigmas.double()]
    x = noise.double() * math.sqrt(1.0 + sig[0] ** 2)
    old = None
    for j in range(len(sig) - 1):
        s, sn = sig[j], sig[j + 1]
        k = S2 / (S2 + s * s)
        D = MU * (1 - k) + x * k
        if sn == 0:
            x = D
        elif old is None:
            x = (sn / s) * x - math.expm1(-math.log(s / sn)) * D
        else:
            h = math.log(s / sn)
            r = math.log(sig[j - 1] / s) / h
            x = (sn / s) * x - math.expm1(-h) * ((1 + 1 / (2 * r)) * D - (1 / (2 * r)) * old)
        old = D
    return x


def test_sampler_on_the_device_matches_its_fp64_restatement(dev, monkeypatch):
    """rel-L2 <= 2e-6 against the fp64 restatement (the fp32 emulation on the CPU gives 2.1e-7; the solver's own truncation
    error is 2.4e-2, so a formula error is four decades above the bound), and the order inequality holds on the device."""
    from seva import sampling as S
    monkeypatch.delenv("SEVA_SOLVER", raising=False)
    noise = torch.randn(XSHAPE, generator=torch.Generator().manual_seed(11))
    disc = S.DDPMDiscretization()

    def solve(solver, steps):
        sm = S.EulerEDMSampler(disc, S.VanillaCFG(), num_steps=steps, verbose=False, device=dev, solver=solver)
        sm.noise_fn = torch.zeros_like  # Euler as an ODE solver (its 1e-6 sigma_hat offset would otherwise inject noise)
        return sm(_analytic(dev), noise.to(dev), SCALE, {}, {}, verbose=False).cpu()

    got = solve("dpmpp2m", 25)
    ref = _dpmpp2m_fp64(noise, disc(25))
    rel = float((got.double() - ref).norm() / ref.norm())
    s0 = float(disc(25)[0])
    exact = MU + (noise.double() * math.sqrt(1 + s0 * s0) - MU) * math.sqrt(S2 / (S2 + s0 * s0))
    err = lambda x: float((x.double() - exact).norm() / exact.norm())  # noqa: E731
    e_ms, e_eu = err(got), err(solve("euler", 50))
    print(f"dpmpp2m 25 steps vs fp64 restatement: {rel:.3e}; error vs exact: dpmpp2m(25) {e_ms:.3e}, euler(50) {e_eu:.3e}")
    assert rel <= 2e-6
    assert e_ms < e_eu


# ------------------------------------------------------------------ whole-step hipGraph
def _runner(net, dev, T, hw, steps, guider, solver=None, eps=None):
    """Like `_loop` of test_model_gpu, but the SAME sampler, cond objects and denoiser callable serve every call of run()."""
    from seva import sampling as S
    from seva import synthetic as synth
    from seva.model import SGMWrapper
    sc = synth.synth_scene(T, (hw, hw), (0,), seed=23)
    disc = S.DDPMDiscretization()
    den = S.DiscreteDenoiser(disc, num_idx=1000, device=dev)
    sampler = S.EulerEDMSampler(disc, guider, num_steps=steps, verbose=False, device=dev, s_churn=0.0, solver=solver)
    wrap = SGMWrapper(net)
    cond = {k: v.to(dev) for k, v in sc["cond"].items()}
    uc = {k: v.to(dev) for k, v in sc["uc"].items()}
    kw = {} if isinstance(guider, S.VanillaCFG) and not isinstance(guider, S.MultiviewCFG) else dict(
        c2w=sc["c2w"].to(dev), K=sc["K"].to(dev), input_frame_mask=sc["input_frame_mask"].to(dev))
    denoiser = lambda x, s, c: den(wrap, x, s, c, num_frames=T)  # noqa: E731

    def run(inference=False):
        if eps is not None:
            it = iter(eps)
            sampler.noise_fn = lambda x: next(it).to(x.device)
        if inference:
            with torch.inference_mode():
                return sampler(denoiser, sc["noise"].to(dev), scale=2.0, cond=cond, uc=uc, verbose=False, **kw).clone()
        return sampler(denoiser, sc["noise"].to(dev), scale=2.0, cond=cond, uc=uc, verbose=False, **kw)

    return run, sampler


@pytest.mark.parametrize("guider_kind", [0, 1, 2])
def test_whole_step_graph_equals_eager_and_history_stays_in_its_trajectory(dev, tiny, guider_kind, monkeypatch):
    from seva import sampling as S
    net, _ = tiny
    T, hw, steps = 4, 16, 6
    mk = lambda: [S.VanillaCFG(), S.MultiviewCFG(1.2), S.MultiviewTemporalCFG(T, 1.2)][guider_kind]  # noqa: E731
    monkeypatch.delenv("SEVA_SOLVER", raising=False)
    monkeypatch.setenv("SEVA_STEPGRAPH", "0")
    monkeypatch.setenv("SEVA_HIPGRAPH", "0")
    run0, s0 = _runner(net, dev, T, hw, steps, mk(), "dpmpp2m")
    ref = run0()
    assert s0._step_graphs.captures == 0 and torch.isfinite(ref).all()
    monkeypatch.setenv("SEVA_STEPGRAPH", "1")
    monkeypatch.setenv("SEVA_HIPGRAPH", "1")
    run1, s1 = _runner(net, dev, T, hw, steps, mk(), "dpmpp2m")
    got = run1()
    assert s1._step_graphs.captures == 1 and s1._step_graphs.graph.replays == steps - 1
    assert torch.equal(got, ref)
    # a second trajectory on the same sampler with the same cond objects: the live graph serves all of its steps
    again = run1()
    assert s1._step_graphs.captures == 1 and s1._step_graphs.graph.replays == 2 * steps - 1
    assert torch.equal(again, ref)
    # ... also when whatever the history buffer held has been destroyed in between
    s1._ms_den.fill_(float("nan"))
    poisoned = run1()
    assert s1._step_graphs.captures == 1 and torch.equal(poisoned, ref)
    # under torch.inference_mode() (how the reference's do_sample calls the sampler)
    run2, s2 = _runner(net, dev, T, hw, steps, mk(), "dpmpp2m")
    got_i = run2(inference=True)
    assert s2._step_graphs.captures == 1 and s2._step_graphs.graph.replays == steps - 1
    assert torch.equal(got_i, ref)
    # the solver is not the Euler solver under another name
    g = torch.Generator().manual_seed(5)
    eps = [torch.randn(T, 4, hw, hw, generator=g) for _ in range(steps)]
    euler, _ = _loop(net, dev, T, hw, steps, eps, mk())
    assert not torch.equal(euler, ref)


def test_default_solver_is_unchanged_on_the_device(dev, tiny, monkeypatch):
    """solver="euler" (and no argument, SEVA_SOLVER unset) is the sampler as it was: no `cfg_multistep` launch, the same bits
    as `EulerEDMSampler` constructed without the new argument (`_loop` of test_model_gpu does that)."""
    from seva import ops
    from seva import sampling as S
    net, _ = tiny
    T, hw, steps = 4, 16, 6
    monkeypatch.delenv("SEVA_SOLVER", raising=False)
    calls = []
    real = ops.cfg_multistep
    monkeypatch.setattr(ops, "cfg_multistep", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    g = torch.Generator().manual_seed(5)
    eps = [torch.randn(T, 4, hw, hw, generator=g) for _ in range(steps)]
    ref, s0 = _loop(net, dev, T, hw, steps, eps, S.MultiviewCFG(1.2))
    assert s0.solver == "euler"
    run, s1 = _runner(net, dev, T, hw, steps, S.MultiviewCFG(1.2), "euler", eps=eps)
    got = run()
    assert torch.equal(got, ref) and not calls
    assert s1._step_graphs.captures == 1 and s1._ms_den is None
