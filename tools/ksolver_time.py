"""Per-step time of the two solvers of `seva.sampling` (euler, dpmpp2m) and the analytic-denoiser error table, on the GPU path.

  python tools/ksolver_time.py [--rounds 6] [--steps 4] [--views 21] [--latent 72]

Part 1: one process, the 1.3 B network with synthetic weights at T = 21, 72 x 72 latents; one sampler per solver, each with its
own trajectory and its own whole-step hipGraph.  After two set-up steps each (eager warm-up, capture) the solvers are timed in
interleaved rounds of `--steps` graph-replayed steps; printed: the median round of each solver and its spread (min .. max).
Part 2: relative L2 error of the final sample against the exact probability-flow solution for an analytic CFG denoiser
(unit-variance Gaussian data, mu_u = 0.3, mu_c = -0.2, scale 2), 25 / 50 / 100 steps -- what the solver's order buys on a problem
with a known answer.  It says nothing about a trained checkpoint."""
import argparse
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stable-virtual-camera_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def step_times(dev, T, hw, rounds, k):
    import bench
    from seva import sampling as S
    from seva import synthetic as synth
    from seva.model import SGMWrapper
    net, _ = bench.build_model(dev)
    net = net.to(dev).eval()
    sc = synth.synth_scene(T, (hw, hw), (0,), seed=23)
    disc = S.DDPMDiscretization()
    den = S.DiscreteDenoiser(disc, num_idx=1000, device=dev)
    wrap = SGMWrapper(net)
    gk = dict(c2w=sc["c2w"].to(dev), K=sc["K"].to(dev), input_frame_mask=sc["input_frame_mask"].to(dev))
    total = 2 + rounds * k
    runs = {}
    for solver in S.SOLVERS:
        sampler = S.EulerEDMSampler(disc, S.MultiviewCFG(1.2), num_steps=total + 1, verbose=False, device=dev, solver=solver)
        cond = {kk: v.to(dev) for kk, v in sc["cond"].items()}
        uc = {kk: v.to(dev) for kk, v in sc["uc"].items()}
        x, s_in, sigmas, _, cond, uc = sampler.prepare_sampling_loop(sc["noise"].to(dev), cond, uc, None)
        runs[solver] = dict(sampler=sampler, x=x, s_in=s_in, sigmas=sigmas, cond=cond, uc=uc, i=0, ms=[],
                            denoise=lambda xx, ss, cc: den(wrap, xx, ss, cc, num_frames=T))

    def advance(r, n):
        for _ in range(n):
            i = r["i"]
            r["x"] = r["sampler"].sampler_step(r["s_in"] * r["sigmas"][i], r["s_in"] * r["sigmas"][i + 1], r["denoise"], r["x"],
                                               2.0, r["cond"], r["uc"], 0.0, **gk)
            r["i"] = i + 1

    with torch.no_grad():
        for r in runs.values():
            advance(r, 2)
            assert r["sampler"]._step_graphs.captures == 1
        for _ in range(rounds):
            for r in runs.values():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                advance(r, k)
                torch.cuda.synchronize()
                r["ms"].append((time.perf_counter() - t0) / k * 1e3)
    for solver, r in runs.items():
        assert torch.isfinite(r["x"]).all()
        ms = r["ms"]
        print(f"[ksolver] {solver:8s} T={T} {hw}x{hw}: median {statistics.median(ms):.2f} ms/step over {rounds} rounds of {k} "
              f"graph-replayed steps (min {min(ms):.2f} .. max {max(ms):.2f})", flush=True)


def error_table(dev):
    from seva import sampling as S
    s2, mu_u, mu_c, scale = 1.0, 0.3, -0.2, 2.0
    mu_g = mu_u + scale * (mu_c - mu_u)
    shape = (4, 4, 6, 5)
    noise = torch.randn(shape, generator=torch.Generator().manual_seed(11))
    mu = torch.cat([torch.full((shape[0],), mu_u), torch.full((shape[0],), mu_c)]).to(dev).view(-1, 1, 1, 1)
    disc = S.DDPMDiscretization()
    s0 = float(disc(25)[0])
    exact = mu_g + (noise.double() * math.sqrt(1 + s0 * s0) - mu_g) * math.sqrt(s2 / (s2 + s0 * s0))

    def denoiser(xx, ss, cc):
        k = (s2 / (s2 + ss * ss)).view(-1, 1, 1, 1)
        return mu * (1 - k) + xx * k

    print("[ksolver] analytic CFG denoiser, rel-L2 of the final sample against the exact solution (GPU path)")
    print("[ksolver] | steps | euler | dpmpp2m |")
    for steps in (25, 50, 100):
        row = []
        for solver in S.SOLVERS:
            sm = S.EulerEDMSampler(disc, S.VanillaCFG(), num_steps=steps, verbose=False, device=dev, solver=solver)
            sm.noise_fn = torch.zeros_like  # Euler as an ODE solver: its 1e-6 sigma_hat offset would otherwise inject noise
            x = sm(denoiser, noise.to(dev), scale, {}, {}, verbose=False).cpu().double()
            row.append(float((x - exact).norm() / exact.norm()))
        print(f"[ksolver] | {steps} | {row[0]:.2e} | {row[1]:.2e} |", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--views", type=int, default=21)
    ap.add_argument("--latent", type=int, default=72)
    ap.add_argument("--no-timing", action="store_true", help="the error table only")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    error_table(dev)
    if not args.no_timing:
        step_times(dev, args.views, args.latent, args.rounds, args.steps)


if __name__ == "__main__":
    main()
