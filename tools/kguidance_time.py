"""What the opt-in guidance controls (`EulerEDMSampler(guidance_interval=, guidance_rescale=)`) cost and buy in time, on the GPU path.

  python tools/kguidance_time.py [--views 21] [--latent 72] [--rounds 5] [--steps 3] [--out profiles/guidance.log]

One process, the 1.3 B network with synthetic weights, device events, every step kind warmed (eager step, then the capture of its
whole-step hipGraph) before anything is timed, the candidates alternating inside every round.
Part 0: the `seva_cfg_rescale_f32` launch alone beside `seva_cfg_combine_f32` on a window's [2n][chw] pair.
Part 1, per window length: ms per guided step with phi = 0 (the sampler with both controls off: the step as tools/kstep_cache_time.py
measures it), per unguided step (the conditional call at batch n) and per guided step with phi = 0.7 (median over the rounds,
min .. max).  The spread of the phi = 0 rounds is the margin against which the phi = 0.7 step is read.
Part 2: steps/s of a 50-step window with the interval off, (0.3, 5] and (0.5, 3], and (0.3, 5] with phi = 0.7; second trajectory of
each sampler (all replays), and the drift: rel-L2 of the final latents against the interval off, same noise.  SYNTHETIC weights:
the drift says how far the arithmetic moves on a random network, nothing about pictures."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stable-virtual-camera_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

LINES = []
PHI = 0.7


def say(msg):
    LINES.append("[kguidance] " + msg)
    print(LINES[-1], flush=True)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernel_times(dev, n, chw, rounds, k=20):
    from seva import ops
    g = torch.Generator().manual_seed(1)
    den2 = torch.randn(2 * n, chw, generator=g).to(dev)
    scale = torch.full((n,), 2.0, device=dev)
    out, mult = torch.empty(n, chw, device=dev), torch.empty(n, device=dev)
    cands = {"cfg_combine": lambda: ops.cfg_combine(den2, scale, out), f"cfg_rescale phi={PHI}": lambda: ops.cfg_rescale(den2, scale, PHI, out, mult)}
    for fn in cands.values():
        fn()
    us = {name: [] for name in cands}
    for _ in range(rounds):
        for name, fn in cands.items():
            us[name].append(timed(lambda: [fn() for _ in range(k)]) / k * 1e3)
    for name, v in us.items():
        say(f"n={n} chw={chw} {name:22s}: median {statistics.median(v):7.1f} us per launch (min {min(v):.1f} .. max {max(v):.1f}, {rounds} rounds "
            f"of {k} back-to-back eager launches; one 256-thread workgroup per frame for cfg_rescale)")


def step_times(net, dev, T, hw, rounds, k):
    import bench
    made = {phi: bench.make_sampler(net, dev, T, hw, 50, 23, time_cond=False) for phi in (0.0, PHI)}
    made[PHI][0].guidance_rescale = PHI
    sampler0, _, noise, cond0, uc0, _ = made[0.0]
    x, s_in, sigmas, _, _, _ = sampler0.prepare_sampling_loop(noise, cond0, uc0, None)
    i = 10  # one sigma of the schedule for every timed step: the time does not depend on it

    def step(phi, guided):
        sampler, denoise, _, cond, uc, gk = made[phi]
        return sampler.sampler_step(s_in * sigmas[i], s_in * sigmas[i + 1], denoise, x, 2.0, cond, uc, 0.0,
                                    **({} if guided else {"guided": False}), **gk)

    kinds = {"guided step, phi = 0": (0.0, True), "unguided step": (0.0, False), f"guided step, phi = {PHI}": (PHI, True)}
    with torch.no_grad():
        for args in kinds.values():  # eager warm-up, then capture + first replay
            step(*args)
            step(*args)
        assert made[0.0][0]._step_graphs.captures == 2 and made[PHI][0]._step_graphs.captures == 1
        assert not made[0.0][0]._step_graphs.disabled and not made[PHI][0]._step_graphs.disabled
        ms = {name: [] for name in kinds}
        for _ in range(rounds):
            for name, args in kinds.items():
                ms[name].append(timed(lambda: [step(*args) for _ in range(k)]) / k)
        assert all(torch.isfinite(step(*args)).all() for args in kinds.values())
    med = {name: statistics.median(v) for name, v in ms.items()}
    base = "guided step, phi = 0"
    for name in kinds:
        say(f"T={T} {hw}x{hw} {name:24s}: median {med[name]:8.2f} ms (min {min(ms[name]):.2f} .. max {max(ms[name]):.2f}, {rounds} rounds "
            f"of {k}); x{med[name] / med[base]:.3f} of the phi = 0 step")
    spread = max(ms[base]) - min(ms[base])
    over = med[f"guided step, phi = {PHI}"] - med[base]
    say(f"T={T} {hw}x{hw} phi = {PHI} over phi = 0: {over:+.2f} ms; spread of the phi = 0 rounds (max - min): {spread:.2f} ms -> "
        f"{'within' if over <= spread else 'EXCEEDS'} that margin")
    return med


def trajectories(net, dev, T, hw, steps, configs, rounds):
    import bench
    runs = {}
    for interval, phi in configs:
        sampler, denoise, noise, cond, uc, gk = bench.make_sampler(net, dev, T, hw, steps, 23, time_cond=False)
        sampler.guidance_interval, sampler.guidance_rescale = interval, phi

        def run(sampler=sampler, denoise=denoise, noise=noise, cond=cond, uc=uc, gk=gk):
            gen = torch.Generator(device=dev)
            gen.manual_seed(7)
            sampler.noise_fn = lambda x: torch.randn(x.shape, generator=gen, device=x.device, dtype=x.dtype)
            return sampler(denoise, noise.clone(), scale=2.0, cond=cond, uc=uc, verbose=False, **gk)

        runs[(interval, phi)] = dict(run=run, sampler=sampler, ms=[])
    with torch.no_grad():
        for r in runs.values():
            r["out"] = r["run"]().clone()  # warm-ups and captures
        for _ in range(rounds):
            for r in runs.values():
                r["ms"].append(timed(r["run"]))
    base = runs[configs[0]]
    base_med = statistics.median(base["ms"])
    for (interval, phi), r in runs.items():
        med = statistics.median(r["ms"])
        sig = r["sampler"]._sigmas_host[:-1]
        guided = steps if interval is None else int(((sig > interval[0]) & (sig <= interval[1])).sum())
        drift = float((r["out"].double() - base["out"].double()).norm() / base["out"].double().norm())
        name = "off" if interval is None else f"({interval[0]:g}, {interval[1]:g}]"
        say(f"T={T} {hw}x{hw} {steps}-step window, guidance_interval {name}, phi {phi:g}: {guided} guided + {steps - guided} unguided steps; "
            f"{steps / med * 1e3:6.2f} steps/s (median of {rounds}: {med / 1e3:.3f} s, min {min(r['ms']) / 1e3:.3f} .. max {max(r['ms']) / 1e3:.3f}); "
            f"x{base_med / med:.2f}; drift of the final latents vs both controls off rel-L2 {drift:.3e} (synthetic weights: says nothing "
            f"about pictures); whole-step graphs {r['sampler']._step_graphs.captures}")
        if phi > 0 and (interval, 0.0) in runs:  # what the rescale alone moves
            same = runs[(interval, 0.0)]["out"].double()
            say(f"T={T} {hw}x{hw} {steps}-step window, guidance_interval {name}: phi {phi:g} against phi 0, final latents rel-L2 "
                f"{float((r['out'].double() - same).norm() / same.norm()):.3e} (scale 2, cfg_min 1.2, synthetic weights)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", default="21", help="window lengths of part 1")
    ap.add_argument("--latent", type=int, default=72)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3, help="timed steps per round and step kind")
    ap.add_argument("--traj-views", type=int, default=21)
    ap.add_argument("--traj-steps", type=int, default=50)
    ap.add_argument("--traj-rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guidance.log"))
    args = ap.parse_args()
    import bench
    dev = torch.device("cuda:0")
    net, _ = bench.build_model(dev)
    net = net.to(dev).eval()
    say(f"1.3 B network, synthetic weights, f16 mode, {torch.cuda.get_device_name(0)}; whole-step hipGraph replays, device events")
    views = [int(v) for v in args.views.split(",") if v]
    for T in views:
        kernel_times(dev, T, 4 * args.latent * args.latent, args.rounds)
    for T in views:
        step_times(net, dev, T, args.latent, args.rounds, args.steps)
    if args.traj_steps > 0:
        trajectories(net, dev, args.traj_views, args.latent, args.traj_steps,
                     [(None, 0.0), ((0.3, 5.0), 0.0), ((0.5, 3.0), 0.0), ((0.3, 5.0), PHI)], args.traj_rounds)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
