"""What the opt-in reuse of deep UNet features (`EulerEDMSampler(cache_interval=, cache_levels=)`) buys, on the GPU path.

  python tools/kstep_cache_time.py [--views 21,41,64] [--latent 72] [--rounds 5] [--steps 3] [--out profiles/step_cache.log]

One process, the 1.3 B network with synthetic weights, device events, every shape and step kind warmed (eager step, then the
capture of its whole-step hipGraph) before anything is timed, the candidates alternating inside every round.
Part 1, per window length: ms per full step and per shallow step of depth 1 and 2 (median over the rounds, min .. max), beside
the FLOPs of each step kind as the library counts them from the shapes of its GEMM / conv / attention launches (one eager,
instrumented step per kind), so the time share stands next to the FLOP share.
Part 2: steps/s of a 50-step window at cache_interval N = 1 (off), 2, 3, 5, second trajectory of each sampler (all replays),
and the drift: rel-L2 of the final latents, cached against uncached, same noise.  SYNTHETIC weights: the drift says how far the
arithmetic moves on a random network, nothing about pictures."""
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


def say(msg):
    LINES.append("[kstep_cache] " + msg)
    print(LINES[-1], flush=True)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def step_times(net, dev, T, hw, rounds, k):
    import bench
    from seva import ops
    sampler, denoise, noise, cond, uc, gk = bench.make_sampler(net, dev, T, hw, 50, 23, time_cond=False)
    x, s_in, sigmas, _, cond, uc = sampler.prepare_sampling_loop(noise, cond, uc, None)
    i = 10  # one sigma of the schedule for every timed step: the time does not depend on it
    kinds = (0, 1, 2)

    def step(kind):
        return sampler.sampler_step(s_in * sigmas[i], s_in * sigmas[i + 1], denoise, x, 2.0, cond, uc, 0.0,
                                    **({"shallow": kind} if kind else {}), **gk)

    eng = net.engine()
    flops = {}
    with torch.no_grad():
        # FLOPs per step kind: one eager step under the library's launch accounting (a full step first: the shallow ones reuse it)
        was_graph, eng.use_graph = eng.use_graph, False
        sampler._step_graphs.disabled = True
        for kind in kinds:
            ops.prof_enable(True)
            step(kind)
            prof = ops.prof_collect()
            ops.prof_enable(False)
            flops[kind] = sum(prof[c]["work"] for c in ("gemm", "conv", "attention"))
        eng.use_graph, sampler._step_graphs.disabled = was_graph, False
        for kind in kinds:  # eager warm-up, then capture + first replay
            step(kind)
            step(kind)
        assert sampler._step_graphs.captures == len(kinds) and not sampler._step_graphs.disabled
        ms = {kind: [] for kind in kinds}
        for _ in range(rounds):
            for kind in kinds:
                ms[kind].append(timed(lambda: [step(kind) for _ in range(k)]) / k)
        assert torch.isfinite(step(0)).all()
    med = {kind: statistics.median(v) for kind, v in ms.items()}
    for kind in kinds:
        name = "full step" if kind == 0 else f"shallow step, depth {kind}"
        say(f"T={T} {hw}x{hw} {name:22s}: median {med[kind]:8.2f} ms (min {min(ms[kind]):.2f} .. max {max(ms[kind]):.2f}, {rounds} rounds "
            f"of {k}); {flops[kind] / 1e12:7.2f} TFLOP; time share {med[kind] / med[0]:.3f}, FLOP share {flops[kind] / flops[0]:.3f}")
    return med


def trajectories(net, dev, T, hw, steps, intervals, levels, rounds):
    import bench
    runs = {}
    for N in intervals:
        sampler, denoise, noise, cond, uc, gk = bench.make_sampler(net, dev, T, hw, steps, 23, time_cond=False)
        sampler.cache_interval, sampler.cache_levels = (N if N >= 2 else 0), levels

        def run(sampler=sampler, denoise=denoise, noise=noise, cond=cond, uc=uc, gk=gk):
            gen = torch.Generator(device=dev)
            gen.manual_seed(7)
            sampler.noise_fn = lambda x: torch.randn(x.shape, generator=gen, device=x.device, dtype=x.dtype)
            return sampler(denoise, noise.clone(), scale=2.0, cond=cond, uc=uc, verbose=False, **gk)

        runs[N] = dict(run=run, sampler=sampler, ms=[])
    with torch.no_grad():
        for r in runs.values():
            r["out"] = r["run"]().clone()  # warm-ups and captures
        for _ in range(rounds):
            for r in runs.values():
                r["ms"].append(timed(r["run"]))
    base = runs[intervals[0]]
    for N, r in runs.items():
        med = statistics.median(r["ms"])
        full = sum(1 for j in range(steps) if N < 2 or j % N == 0 or j == steps - 1)
        drift = float((r["out"].double() - base["out"].double()).norm() / base["out"].double().norm())
        say(f"T={T} {hw}x{hw} {steps}-step window, cache_interval {N}, depth {levels}: {full} full + {steps - full} shallow steps; "
            f"{steps / med * 1e3:6.2f} steps/s (median of {rounds}: {med / 1e3:.3f} s, min {min(r['ms']) / 1e3:.3f} .. max {max(r['ms']) / 1e3:.3f}); "
            f"x{base_speed(base, med):.2f}; drift of the final latents vs interval {intervals[0]} rel-L2 {drift:.3e} (synthetic weights: says nothing "
            f"about pictures); whole-step graphs {r['sampler']._step_graphs.captures}")


def base_speed(base, med):
    return statistics.median(base["ms"]) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", default="21,41,64", help="window lengths of part 1")
    ap.add_argument("--latent", type=int, default=72)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3, help="timed steps per round and step kind")
    ap.add_argument("--traj-views", type=int, default=21)
    ap.add_argument("--traj-steps", type=int, default=50)
    ap.add_argument("--traj-rounds", type=int, default=2)
    ap.add_argument("--intervals", default="1,2,3,5")
    ap.add_argument("--levels", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_cache.log"))
    args = ap.parse_args()
    import bench
    dev = torch.device("cuda:0")
    net, _ = bench.build_model(dev)
    net = net.to(dev).eval()
    say(f"1.3 B network, synthetic weights, f16 mode, {torch.cuda.get_device_name(0)}; whole-step hipGraph replays, device events")
    for T in (int(v) for v in args.views.split(",") if v):
        step_times(net, dev, T, args.latent, args.rounds, args.steps)
    if args.traj_steps > 0:
        trajectories(net, dev, args.traj_views, args.latent, args.traj_steps, [int(v) for v in args.intervals.split(",")],
                     args.levels, args.traj_rounds)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
