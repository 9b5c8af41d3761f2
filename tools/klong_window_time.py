#!/usr/bin/env python3
"""What a window of 33 to 90 views costs on the device:

    python tools/klong_window_time.py [--iters N] [--rounds R] [--skip-network] [--network-T 21,41,53,64,90] [--out FILE]

A. The temporal-attention launches of a step (the four levels of the 1.3B network at 576 x 576: hw 5184 / 1296 / 324 / 81 pixels with
   5 / 10 / 20 / 20 heads, CFG batch 2, the engine's strided layout and pre-scaled q) at T = 33, 41, 53, 64 on BOTH routes of
   32 < lq <= 64 -- knob attn_short2 = 0: attn_kernel<4, 64> on the three-buffer ring; 1: attn_kernel<2, 64> on one buffer -- alternating
   in one process, device events, after a warm-up of every shape and route.  Per shape: the median over the rounds and the spread
   (max - min) each route shows over its own rounds, and whether their outputs are equal bits.  T = 21 (attn_kernel<1, 32>) is timed in
   the same run as the yardstick.
   The rule of the default: the two-wave route is faster at levels 0 and 1 for T = 41 and T = 64 by more than the four-wave route's
   own spread there.
B. One call of the 1.3B network (CFG batch 2T, synthetic weights) at 576 x 576 for T = 21, 41, 53, 64, 90: eager and replayed
   (hipGraph), the per-class split of seva_prof_collect over one eager call, the arena's size.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stable-virtual-camera_amd"))
import torch  # noqa: E402

from seva import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=40)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--skip-network", action="store_true")
ap.add_argument("--network-T", default="21,41,53,64,90")
ap.add_argument("--out", default=None, help="also append every line to this file")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("klong_window_time.py: needs the GPU (a timing taken elsewhere says nothing)")
dev = torch.device("cuda:0")
LOG2E = 1.4426950408889634
LEVELS = [(0, 5184, 5), (1, 1296, 10), (2, 324, 20), (3, 81, 20)]


def say(line=""):
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def temporal(T, S, H, seed):
    B, C = 2, 64 * H
    g = torch.Generator(device=dev).manual_seed(seed)
    qkv = torch.randn(B * T, S, 3 * C, device=dev, generator=g)
    qkv[..., :C] *= 0.125 * LOG2E
    qkv = qkv.half()
    out = torch.empty(B * T, S, C, device=dev, dtype=torch.float16)

    def call():
        ops.attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], out, nb0=B, nb1=S, heads=H, lq=T, lk=T,
                      q_strides=(T * S * 3 * C, 3 * C, S * 3 * C), k_strides=(T * S * 3 * C, 3 * C, S * 3 * C),
                      o_strides=(T * S * C, C, S * C), q_prescaled=True)
    return call, out


def timeit(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us per launch


say(f"# tools/klong_window_time.py --iters {args.iters} --rounds {args.rounds}   ({torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')})")
say("== A. temporal attention, one launch, us: median over the rounds [spread = max - min over the route's own rounds]")
say("level    hw heads   T | 4-wave ring (knob 0)   | 2-wave 1 buffer (knob 1) | 2-wave / 4-wave | equal bits | faster beyond spread")
verdict = {}
for lvl, S, H in LEVELS:
    call, out = temporal(21, S, H, 1)
    call()
    torch.cuda.synchronize()
    ys = [timeit(call, args.iters) for _ in range(args.rounds)]
    say(f"{lvl:5d} {S:5d} {H:5d}  21 | {statistics.median(ys):8.1f} [{max(ys) - min(ys):5.1f}]  attn_kernel<1, 32>: the yardstick")
    for T in (33, 41, 53, 64):
        call, out = temporal(T, S, H, T)
        res = {}
        for knob in (0, 1):  # warm-up of both routes, and their outputs
            ops.set_knob("attn_short2", knob)
            out.fill_(float("nan"))
            call()
            torch.cuda.synchronize()
            res[knob] = out.clone()
        same = bool(torch.equal(res[0], res[1])) and bool(torch.isfinite(res[0]).all())
        del res
        ts = {0: [], 1: []}
        for _ in range(args.rounds):
            for knob in (0, 1):
                ops.set_knob("attn_short2", knob)
                ts[knob].append(timeit(call, args.iters))
        m0, m1 = statistics.median(ts[0]), statistics.median(ts[1])
        s0, s1 = max(ts[0]) - min(ts[0]), max(ts[1]) - min(ts[1])
        faster = m0 - m1 > s0
        verdict[(lvl, T)] = faster and same
        say(f"{lvl:5d} {S:5d} {H:5d} {T:3d} | {m0:8.1f} [{s0:5.1f}]       | {m1:8.1f} [{s1:5.1f}]         | {m1 / m0:8.3f}        | "
            f"{'yes' if same else 'NO':10s} | {'yes' if faster else 'no'}")
    del call, out
    torch.cuda.empty_cache()
ops.set_knob("attn_short2", -1)
rule = all(verdict[k] for k in ((0, 41), (0, 64), (1, 41), (1, 64)))
say(f"rule of the default (levels 0 and 1, T = 41 and 64, faster beyond the four-wave route's spread, equal bits): "
    f"{'the two-wave route qualifies' if rule else 'the two-wave route does NOT qualify'}")

if args.skip_network:
    sys.exit(0)

# ---------------------------------------------------------------------------------------------------------------- B. the network
from seva import synthetic as synth  # noqa: E402
from seva.model import Seva, SevaParams  # noqa: E402

say()
say("== B. one call of the 1.3B network at 576 x 576 (latent 72 x 72, CFG batch 2T), ms")
with torch.device("meta"):
    net = Seva(SevaParams())
sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 0)
net.load_state_dict(sd, strict=True, assign=True)
net = net.to(dev).eval()
del sd
hw = 72
rows = []
for T in [int(v) for v in args.network_T.split(",")]:
    eng = net.engine()
    eng._graphs.clear()
    eng.arena.bufs.clear()  # the arena then holds this T's buffers only
    torch.cuda.empty_cache()
    sc = synth.synth_scene(T, (hw, hw), (0,), seed=100 + T)
    x = torch.randn(2 * T, 4, hw, hw, generator=torch.Generator().manual_seed(T)).to(dev)
    c = {k: torch.cat((sc["uc"][k], sc["cond"][k]), 0).to(dev) for k in ("crossattn", "concat", "dense_vector")}
    t = torch.full((2 * T,), 979, dtype=torch.int64, device=dev)
    a = (x, c["concat"], t, c["crossattn"], c["dense_vector"], T)
    with torch.no_grad():
        y = eng.forward(*a)  # warm-up: fills the arena
        torch.cuda.synchronize()
        assert torch.isfinite(y).all()
        eager = statistics.median(timeit(lambda: eng.forward(*a), 2) / 1e3 for _ in range(3))
        eng.forward_graphed(*a)  # capture
        torch.cuda.synchronize()
        replay = statistics.median(timeit(lambda: eng.forward_graphed(*a), 2) / 1e3 for _ in range(3))
        ops.prof_enable(True)
        ops.prof_collect()
        eng.forward(*a)
        prof = ops.prof_collect()
        ops.prof_enable(False)
    cls = {k: v["ms"] for k, v in prof.items() if v["launches"]}
    tot = sum(cls.values())
    arena = eng.arena.nbytes() / 2 ** 30
    say(f"T={T:3d}: eager {eager:8.2f}  replayed {replay:8.2f}  arena {arena:6.2f} GiB  | per class (one eager call, {tot:.2f} ms in kernels): "
        + ", ".join(f"{k} {v:.2f} ({100 * v / tot:.0f} %)" for k, v in sorted(cls.items(), key=lambda kv: -kv[1])))
    rows.append((T, eager, replay, arena))
base = rows[0]
for T, eager, replay, arena in rows[1:]:
    say(f"T={T:3d} against T={base[0]}: replayed x{replay / base[2]:.2f} for x{T / base[0]:.2f} the views; arena x{arena / base[3]:.2f}")
