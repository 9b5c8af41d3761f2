"""Goldens of the STOCHASTIC Euler sampler, s_churn > 0 (dev container only; CPU, under a minute).

    PYTHONDONTWRITEBYTECODE=1 python oracle/make_goldens_churn.py

Sibling of `make_goldens_nonsquare.py`: runs the REFERENCE's `EulerEDMSampler.__call__` (imported read-only exactly as
`oracle/make_goldens.py` does, whose `_patch_randn`, `synth`, `rnd` and `save` are reused) with recorded eps.

  g14_churn_analytic   every case of tests/churn_cases.py (`CASES`) with each of the three guiders on the analytic CFG
                       denoiser, latent (4, 4, 6, 5).  Per case: the settings and the eps; per case and guider the output `y`,
                       the `gamma` the reference handed to each `sampler_step` (recorded by wrapping it, not re-derived), the
                       fp32 `sigma_hat` each step's denoiser call saw, and `ref_vs_fp64`: rel-L2 between the reference's fp32
                       output and the fp64 restatement `churn_cases.restate_fp64` (fp32 per-step scalars, fp64 latents).
  g14_churn_tiny       the recipe of g7_loop_tiny (T = 4, 16x16 latent, scene seed 23, MultiviewCFG(1.2), scale 2.0) on the
                       tiny network with 6 steps, s_churn = 1.5, s_tmin = 1.0, s_tmax = 60.0, s_noise = 1.003: output, eps, gammas.

Reference call sites: seva/sampling.py:347-368 (sampler_step), 370-405 (__call__).
"""

from __future__ import annotations

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as mg  # noqa: E402  (imports the reference + seva.synthetic)

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
sys.path.insert(0, mg.ROOT)
import churn_cases as C  # noqa: E402  (imports neither `seva`)

rsamp, rmodel, synth = mg.rsamp, mg.rmodel, mg.synth
FILE_LIMIT = 1 << 20


def _recording(sampler):
    """Wraps the instance's `sampler_step`: -> the list that receives the gamma of every call."""
    gammas = []
    inner = sampler.sampler_step

    def step(sigma, next_sigma, denoiser, x, scale, cond, uc, gamma=0.0, **kw):
        gammas.append(float(gamma))
        return inner(sigma, next_sigma, denoiser, x, scale, cond, uc, gamma, **kw)

    sampler.sampler_step = step
    return gammas


def _run_reference(sampler, denoiser, x0, eps, scale, cond, uc, **kw):
    orig = mg._patch_randn(eps)
    try:
        return sampler(denoiser, x0.clone(), scale=scale, cond=cond, uc=uc, verbose=False, **kw)
    finally:
        rsamp.torch.randn_like = orig


@torch.no_grad()
def g14_churn_analytic():
    disc = rsamp.DDPMDiscretization()
    v = C.views(synth)
    x0 = C.noise()
    out = dict(noise=x0, c2w=v["c2w"], K=v["K"], mask=v["input_frame_mask"])
    worst = 0.0
    for name in C.CASES:
        st = C.settings(name, disc)
        steps = st["steps"]
        eps = C.eps_list(steps)
        out[f"{name}__eps"] = torch.stack(eps)
        for k, val in st.items():
            out[f"{name}__{k}"] = torch.tensor(val, dtype=torch.float64).numpy()
        for kind in C.GUIDERS:
            sampler = rsamp.EulerEDMSampler(disc, C.make_guider(rsamp, kind), num_steps=steps, verbose=False, device="cpu",
                                            s_churn=st["s_churn"], s_tmin=st["s_tmin"], s_tmax=st["s_tmax"], s_noise=st["s_noise"])
            gammas, seen = _recording(sampler), []

            def denoiser(xx, ss, cc):
                seen.append(ss[0].clone())
                return C.denoiser(xx, ss, cc)

            y = _run_reference(sampler, denoiser, x0, eps, C.SCALE, {}, {}, **C.guider_kwargs(kind, v))
            assert y.dtype == torch.float32 and len(gammas) == steps == len(seen)
            ref64 = C.restate_fp64(x0, eps, disc(steps), gammas, st["s_noise"], C.frame_scale(kind, v))
            rel = C.rel_l2(y, ref64)
            worst = max(worst, rel)
            print(f"  {name:8s} {kind:9s} gamma {[round(g, 4) for g in gammas]}  reference fp32 vs fp64 restatement: {rel:.3e}", flush=True)
            pre = f"{name}__{kind}__"
            out[pre + "y"], out[pre + "gamma"] = y, torch.tensor(gammas, dtype=torch.float64)
            out[pre + "sigma_hat"], out[pre + "ref_vs_fp64"] = torch.stack(seen), torch.tensor(rel, dtype=torch.float64).numpy()
    print(f"  largest ref_vs_fp64: {worst:.3e}")
    mg.save(C.GOLDEN, **out)


@torch.no_grad()
def g14_churn_tiny():
    t = C.TINY
    T, hw, steps = t["T"], t["hw"], t["steps"]
    net = mg.load_synth(rmodel.Seva(rmodel.SevaParams(model_channels=64)))
    disc = rsamp.DDPMDiscretization()
    den = rsamp.DiscreteDenoiser(disc, num_idx=1000, device="cpu")
    sampler = rsamp.EulerEDMSampler(disc, rsamp.MultiviewCFG(C.CFG_MIN), num_steps=steps, verbose=False, device="cpu",
                                    s_churn=t["s_churn"], s_tmin=t["s_tmin"], s_tmax=t["s_tmax"], s_noise=t["s_noise"])
    gammas = _recording(sampler)
    sc = synth.synth_scene(T, (hw, hw), (0,), seed=t["scene_seed"])
    eps = C.eps_list(steps, (T, 4, hw, hw), t["eps_seed"])
    wrap = rmodel.SGMWrapper(net)
    y = _run_reference(sampler, lambda xx, ss, cc: den(wrap, xx, ss, cc, num_frames=T), sc["noise"], eps, t["scale"],
                       sc["cond"], sc["uc"], c2w=sc["c2w"], K=sc["K"], input_frame_mask=sc["input_frame_mask"])
    print(f"  tiny loop gamma {[round(g, 4) for g in gammas]}")
    mg.save(C.GOLDEN_TINY, y=y, eps=torch.stack(eps), gamma=torch.tensor(gammas, dtype=torch.float64),
            **{k: torch.tensor(val, dtype=torch.float64).numpy() for k, val in t.items()})


def main():
    os.makedirs(mg.GOLD, exist_ok=True)
    print("G14 churn, analytic denoiser"); g14_churn_analytic()
    print("G14 churn, tiny network"); g14_churn_tiny()
    for name in (C.GOLDEN, C.GOLDEN_TINY):
        size = os.path.getsize(os.path.join(mg.GOLD, name + ".npz"))
        assert size <= FILE_LIMIT, f"{name}: {size} bytes is over the limit for a committed file"


if __name__ == "__main__":
    main()
