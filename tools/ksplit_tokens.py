"""The split-precision table of DESIGN.md section 2, one row per token set (the default, the default plus each further class, `all`).

  python tools/ksplit_tokens.py --predict     CPU: the fp32 oracle with fp16 operands, the set's classes carried as hi + lo, against the
                                               unmodified oracle on BASELINE config 1 (1.3B synthetic weights) -- the "predicted" column
  python tools/ksplit_tokens.py               GPU: rel-L2 / worst latent of the T = 21, 72 x 72 forward against the reference's own output
                                               (tests/golden/g9_T21_forward.npz, the metric of tests/test_headline_gpu.py) and ms per network
                                               call (B = 42, hipGraph replay, HIP events, median of --reps) in one process, weights re-packed
                                               per set -- the "measured" columns
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stable-virtual-camera_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

DEFAULT = "stem,head,skip_deep"
SETS = [DEFAULT] + [f"{DEFAULT},{t}" for t in ("conv", "resample", "proj_in", "proj_out", "qkv", "ff")] + ["stem,head,skip", "all"]


def predict():
    import pytest
    import test_split_operands_cpu as TS
    from conftest import load_golden, rel_l2
    from oracle import seva_ref as O
    from seva import synthetic as synth
    from seva._engine import parse_split
    from seva.model import Seva, SevaParams

    g = load_golden("g4_full_forward")
    T = int(g["T"])
    with torch.device("meta"):
        net = Seva(SevaParams())
    sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 0)
    c = {k: g[k] for k in ("crossattn", "concat", "dense_vector")}
    torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 16)))
    with torch.no_grad():
        exact = O.sgm_wrapper_forward(sd, g["x"], g["t"], c, num_frames=T)
    for s in SETS:
        mp = pytest.MonkeyPatch()
        emu = TS._emulate(mp, sd, lambda: O.sgm_wrapper_forward(sd, g["x"], g["t"], c, num_frames=T), tuple(parse_split(s)))
        per = [rel_l2(emu[i], exact[i]) for i in range(exact.shape[0])]
        print(f"predict {s:32s} rel-L2 {rel_l2(emu, exact):.3e} worst latent {max(per):.3e}", flush=True)


def measure(reps):
    from conftest import load_golden, rel_l2
    from seva.model import SGMWrapper
    from test_headline_gpu import FORWARD_SEEDS, _wrapper_inputs
    from test_model_gpu import _build

    dev = torch.device("cuda:0")
    net, _ = _build("full", dev)
    T = 21
    ref = load_golden("g9_T21_forward")["y"]
    x, t, c = _wrapper_inputs(T, FORWARD_SEEDS[T])
    x, t, c = x.to(dev), t.to(dev), {k: v.to(dev) for k, v in c.items()}
    for s in SETS:
        net.set_precision("f16", split=s)
        wrap = SGMWrapper(net)
        y = wrap(x, t, c, num_frames=T)  # (first call of a signature: warm-up + capture)
        y = wrap(x, t, c, num_frames=T).cpu()
        per = [rel_l2(y[i], ref[i]) for i in range(y.shape[0])]
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            wrap(x, t, c, num_frames=T)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        print(f"measure {s:32s} rel-L2 {rel_l2(y, ref):.3e} worst latent {max(per):.3e}  network call {ms[len(ms) // 2]:.2f} ms "
              f"(min {ms[0]:.2f}, max {ms[-1]:.2f}, {reps} reps)", flush=True)
        net._engine = None
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--predict", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    predict() if a.predict else measure(a.reps)
