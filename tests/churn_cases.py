"""Shared by tests/test_sampler_churn_cpu.py, tests/test_sampler_churn_gpu.py and oracle/make_goldens_churn.py: the cases of
the stochastic Euler sampler (s_churn > 0), the analytic CFG denoiser, the fp64 restatement of one trajectory with its three
mutants, and the counters the whole-step graph protocol must show for a gamma sequence.  Imports neither the product nor the
reference (the generator loads it beside the reference's `seva` package); what needs `seva` gets it as an argument."""
import math

import torch

S2, MU_U, MU_C, SCALE = 1.0, 0.3, -0.2, 2.0  # analytic CFG denoiser: data N(mu, s^2) with s = 1 (tests/test_solver_dpmpp2m_gpu.py)
XSHAPE = (4, 4, 6, 5)
CFG_MIN = 1.2
GUIDERS = ("vanilla", "multiview", "temporal")
GOLDEN, GOLDEN_TINY = "g14_churn_analytic", "g14_churn_tiny"
SCENE_SEED, NOISE_SEED, EPS_SEED = 1400, 1401, 1402

# name -> (steps, s_churn, s_tmin, s_tmax, s_noise); None = a bound that `settings` places at one schedule sigma
CASES = {
    "all": (12, 3.0, 0.0, float("inf"), 1.0),      # gamma = 0.25 on every step
    "window": (12, 3.0, 0.5, 50.0, 1.003),         # the first steps lie above the window
    "capped": (12, 40.0, 0.5, 50.0, 1.003),        # gamma at its cap sqrt(2) - 1
    "inner": (8, 2.0, 1.0, 30.0, 0.9),             # the trajectory enters the window
    "edge_hi": (8, 2.0, 0.0, None, 1.0),           # s_tmax one double below sigmas[2]: rounds to it in fp32
    "edge_lo": (8, 2.0, None, float("inf"), 1.0),  # s_tmin one double above sigmas[5]: rounds to it in fp32
}
# the tiny-network loop (recipe of g7_loop_tiny: T = 4, 16x16 latent, scene seed 23, MultiviewCFG(1.2), scale 2.0)
TINY = dict(T=4, hw=16, steps=6, s_churn=1.5, s_tmin=1.0, s_tmax=60.0, s_noise=1.003, scene_seed=23, eps_seed=1499, scale=2.0)


def settings(name, discretization):
    """-> dict(steps, s_churn, s_tmin, s_tmax, s_noise) of one case; `discretization(steps)` gives the fp32 schedule."""
    steps, s_churn, s_tmin, s_tmax, s_noise = CASES[name]
    if s_tmax is None:
        s_tmax = math.nextafter(float(discretization(steps)[2]), 0.0)
    if s_tmin is None:
        s_tmin = math.nextafter(float(discretization(steps)[5]), math.inf)
    return dict(steps=steps, s_churn=s_churn, s_tmin=s_tmin, s_tmax=s_tmax, s_noise=s_noise)


def denoiser(xx, ss, cc):
    """[uncond ; cond] halves of the analytic denoiser D = mu (1 - k) + x k, k = s^2 / (s^2 + sigma^2)."""
    n = xx.shape[0] // 2
    mu = torch.cat([torch.full((n,), MU_U), torch.full((n,), MU_C)]).to(device=xx.device, dtype=xx.dtype).view(-1, 1, 1, 1)
    k = (S2 / (S2 + ss * ss)).view(-1, 1, 1, 1)
    return mu * (1 - k) + xx * k


def denoiser_on(device, n=XSHAPE[0]):
    """`denoiser` with mu built once on `device`: nothing in it copies from the host, so a stream capture can record it."""
    mu = torch.cat([torch.full((n,), MU_U), torch.full((n,), MU_C)]).to(device).view(-1, 1, 1, 1)

    def fn(xx, ss, cc):
        k = (S2 / (S2 + ss * ss)).view(-1, 1, 1, 1)
        return mu * (1 - k) + xx * k

    return fn


def views(synth):
    """Poses of `synth.synth_scene` with frame 2 made a "close frame" of the input frame (as g6_guiders does)."""
    sc = synth.synth_scene(XSHAPE[0], XSHAPE[2:], (0,), seed=SCENE_SEED)
    c2w = sc["c2w"].clone()
    c2w[2] = c2w[0]
    return {"c2w": c2w, "K": sc["K"], "input_frame_mask": sc["input_frame_mask"]}


def noise():
    return torch.randn(XSHAPE, generator=torch.Generator().manual_seed(NOISE_SEED))


def eps_list(steps, shape=XSHAPE, seed=EPS_SEED):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(shape, generator=g) for _ in range(steps)]


def make_guider(S, kind):
    """`S` is a sampling module: the project's or the reference's."""
    return {"vanilla": S.VanillaCFG, "multiview": lambda: S.MultiviewCFG(CFG_MIN),
            "temporal": lambda: S.MultiviewTemporalCFG(XSHAPE[0], CFG_MIN)}[kind]()


def guider_kwargs(kind, v):
    return {} if kind == "vanilla" else dict(v)


def frame_scale(kind, v):
    """The per-frame guidance weight of each guider, fp64 (n,), from the oracle's pinned restatement of the scale rules."""
    from oracle import sampling_ref as SR
    n = XSHAPE[0]
    if kind == "vanilla":
        return torch.full((n,), SCALE, dtype=torch.float64)
    s = SCALE if kind == "multiview" else SR.temporal_scale(SCALE, CFG_MIN, v["input_frame_mask"], n)
    return SR.multiview_scale(s, CFG_MIN, v["c2w"], v["K"], v["input_frame_mask"]).double().reshape(n)


def step_scalars(sigmas, i, gamma, n=XSHAPE[0]):
    """(sigma_hat, sqrt(sigma_hat^2 - sigma^2), dt) of step i as fp32 (n,) vectors, formed as the reference's sampler_step forms
    them from `s_in * sigmas[i]`.  The fp32 values are the specification: at gamma = 0 and sigma = 84.9 the 1e-6 is below half
    an ulp, so the noise scale is 0, where fp64 scalars would give 0.013."""
    assert sigmas.dtype == torch.float32
    s_in = torch.ones(n, dtype=torch.float32)
    sigma, nxt = s_in * sigmas[i], s_in * sigmas[i + 1]
    sigma_hat = sigma * (gamma + 1.0) + 1e-6
    return sigma_hat, (sigma_hat ** 2 - sigma ** 2) ** 0.5, nxt - sigma_hat


MUTANTS = ("s_noise_ignored", "gamma_ignored", "linear_noise_scale")


def restate_fp64(x0, eps, sigmas, gammas, s_noise, fscale, mutant=None):
    """One trajectory of the reference's EulerEDMSampler on the analytic denoiser: per-step scalars in fp32 (`step_scalars`),
    everything latent-sized in fp64.  `sigmas` is the fp32 schedule with the trailing 0, `gammas` what each step was given,
    `fscale` the per-frame guidance weight.  `mutant` names one deliberate error (MUTANTS)."""
    assert mutant is None or mutant in MUTANTS
    col = lambda v: v.double().view(-1, 1, 1, 1)  # noqa: E731
    x = x0.double() * torch.sqrt(1.0 + sigmas[0] ** 2.0).double()
    for i, gamma in enumerate(gammas):
        gamma = 0.0 if mutant == "gamma_ignored" else float(gamma)
        sigma_hat, nscale, dt = step_scalars(sigmas, i, gamma, x.shape[0])
        if mutant == "linear_noise_scale":
            nscale = sigma_hat - sigmas[i]
        e = eps[i].double() * (1.0 if mutant == "s_noise_ignored" else s_noise)
        x = x + e * col(nscale)
        sh = sigma_hat.double()
        u, c = denoiser(torch.cat([x, x]), torch.cat([sh, sh]), {}).chunk(2)
        den = u + col(fscale) * (c - u)
        x = x + col(dt) * ((x - den) / col(sh))
    return x


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm())


def runs_of(gammas):
    """Lengths of the maximal runs of equal gamma."""
    out = []
    for j, g in enumerate(gammas):
        if j and float(g) == float(gammas[j - 1]):
            out[-1] += 1
        else:
            out.append(1)
    return out


def expected_counters(gammas):
    """What the whole-step graph protocol shows after the steps `gammas` (of one trajectory, or of several in a row on one
    sampler with the same cond objects: the key differs between two steps exactly where gamma does).  Each maximal run of equal
    gamma of length L: one eager warm-up, one capture if L >= 2, L - 1 replays.
    -> (warm-ups, captures, replays of the live graph or None when the last run left none)."""
    runs = runs_of(gammas)
    return len(runs), sum(1 for n in runs if n >= 2), (runs[-1] - 1 if runs[-1] >= 2 else None)
