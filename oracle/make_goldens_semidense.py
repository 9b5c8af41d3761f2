"""Goldens of the SEMI-DENSE regime: per-pass window lengths and windows of 41 to 90 views (dev container only; about ten
minutes of CPU).

    PYTHONDONTWRITEBYTECODE=1 python oracle/make_goldens_semidense.py [--only plans,g15_T41,...] [--no-parity]

Sibling of `make_goldens_nonsquare.py`: runs the REFERENCE (CPU fp32, imported read-only exactly as `oracle/make_goldens.py`
and `oracle/make_goldens_next.py` do) and stores OUTPUTS only.

  g15_semidense_plans.json   anchors, [T1, T2] and both passes' window lists of eight trajectories with nine or more input
                             views, from the reference's `infer_prior_stats` / `infer_prior_inds` / `chunk_input_and_test` in
                             `run_one_scene`'s composition (seva/eval.py:1653-1885; `g10_two_pass` of make_goldens_next.py with
                             the window length of each pass taken from what `infer_prior_stats` writes back).  Cameras:
                             `seva.synthetic.orbit_c2w(n)`, input views first.
  g15_T41_forward.npz        one SGMWrapper call each (seva/model.py:176-234), name-keyed synthetic 1.3B weights (seed 0), 16 x 16
  g15_T64_forward.npz        latent, the `[uncond; cond]` recipe of make_goldens_nonsquare.py with the INPUT SLOTS of a real plan
  g15_T65_forward.npz        (stored as `input_slots`): the first pass of 32 inputs + 9 / 32 / 33 anchors (T = 41: the 168-frame
  g15_T90_forward.npz        plan; 64: `--T 64,21`; 65: `num_prior_frames` = 33) and the one-pass window of `--T 90` (32 inputs,
                             58 targets).  The whole output is stored (T = 90: 180 latents).

Second stage (a child process, which imports this repository's package instead of the reference): for every stored forward
the ideal machine of tests/test_split_operands_cpu.py -- the fp32 oracle with every GEMM / conv operand rounded to fp16 -- against the
stored reference output, (a) with the engine's default split classes (`stem`, `head`, `skip_deep`) and (b) all-f16.  Both figures
go to profiles/semidense_parity.log.  (a) is what NET_TOL has to hold against on the device.
"""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden")
LOG = os.path.join(ROOT, "profiles", "semidense_parity.log")
HW = 16
NET_TOL = 1e-3

# name -> (n frames, input views, chunk_strategy, T, options)
PLANS = {
    "in9_n100": (100, 9, "interp", 21, {}),
    "in9_n330": (330, 9, "interp", 21, {}),
    "in16_n96": (96, 16, "interp", 21, {}),
    "in32_n168": (168, 32, "interp", 21, {}),
    "in12_n120_gt": (120, 12, "interp-gt", 21, {}),
    "in32_n168_gt": (168, 32, "interp-gt", 21, {}),
    "in32_n168_T96": (168, 32, "interp", [96, 21], {}),
    "in16_n96_ratio": (96, 16, "interp", 21, {"num_prior_frames_ratio": 1.2}),
}
# name -> (T, seed); x is drawn from seed + 1.  No collision with 400 / 500 / 600 / 701 / 702 / 810 .. 841.
FORWARDS = {"g15_T41": (41, 1510), "g15_T64": (64, 1520), "g15_T65": (65, 1530), "g15_T90": (90, 1540)}
FILE_LIMIT = 1 << 20


# ---------------------------------------------------------------------------------------------------------------- stage 1: reference
def semidense_plan(reval, synth, n, n_in, strategy, T, options, first_pass="gt-nearest"):
    opts = {"sampler_verbose": False, **options, "chunk_strategy": strategy}
    vd = {"T": T, "options": opts}
    ins = list(range(n_in))
    npf = reval.infer_prior_stats(T, n_in, n - n_in, vd)
    T1, T2 = vd["T"] if isinstance(vd["T"], (list, tuple)) else (T, T)
    c_all = synth.orbit_c2w(n)
    prior = [int(v) for v in reval.infer_prior_inds(c_all, npf, list(ins), opts)]
    p1 = reval.chunk_input_and_test(T1, c_all[ins], c_all[prior], list(ins), list(prior), opts, task="img2trajvid",
                                    chunk_strategy=first_pass, gt_input_inds=list(range(n_in)))
    order = np.argsort(ins + prior).tolist()
    pool = np.array(ins + prior)[order].tolist()
    test = [i for i in range(n) if i not in ins]
    p2 = reval.chunk_input_and_test(T2, c_all[pool], c_all[test], list(pool), list(test), opts, task="img2trajvid",
                                    chunk_strategy=strategy, gt_input_inds=[order.index(i) for i in range(n_in)])

    def rec(p):
        return {"chunks": p[0], "input_inds": p[1], "input_sels": p[2], "test_inds": p[3], "test_sels": p[4]}
    return {"n": n, "input_ids": ins, "T": T, "chunk_strategy": strategy, "first_pass_strategy": first_pass, "options": options,
            "num_prior_frames": int(npf), "prior_inds": prior, "T_passes": [int(T1), int(T2)], "pass1": rec(p1), "pass2": rec(p2)}


def plans_golden(reval, synth):
    out = {}
    for name, (n, n_in, strategy, T, options) in PLANS.items():
        out[name] = g = semidense_plan(reval, synth, n, n_in, strategy, T, options)
        print(f"  g15 {name}: T {g['T_passes']}, {len(g['prior_inds'])} prior frames, pass 1 {len(g['pass1']['chunks'])} windows, "
              f"pass 2 {len(g['pass2']['chunks'])} windows", flush=True)
    path = os.path.join(GOLD, "g15_semidense_plans.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"), default=lambda v: v.tolist() if hasattr(v, "tolist") else int(v))
    print(f"  wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


def input_slots_of(reval, synth, T):
    """the slots the 32 input views take in the window of T views that the reference plans"""
    n_in = 32
    ins = list(range(n_in))
    if T == 90:  # `--T 90`: one forward over 32 inputs + 58 targets (use_traj_prior = False, strategy "gt")
        c_all = synth.orbit_c2w(T)
        test = list(range(n_in, T))
        p = reval.chunk_input_and_test(T, c_all[ins], c_all[test], list(ins), list(test), {"sampler_verbose": False}, task="img2img",
                                       chunk_strategy="gt", gt_input_inds=list(ins))
    else:
        Targ, options = {41: (21, {}), 64: ([64, 21], {}), 65: (21, {"num_prior_frames": 33})}[T]
        g = semidense_plan(reval, synth, 168, n_in, "interp", Targ, options)
        assert g["T_passes"][0] == T, (T, g["T_passes"])
        p = [g["pass1"][k] for k in ("chunks", "input_inds", "input_sels", "test_inds", "test_sels")]
    assert len(p[0]) == 1, "one window"
    in_sels, te_sels, in_maps, _ = reval.pad_indices(list(p[2][0]), list(p[4][0]), T=T, padding_mode="last")
    slots = [s for s in range(T) if in_maps[s] != -1]
    assert len(slots) == n_in and len(in_sels) + len(te_sels) == T
    return slots


def semidense_inputs(synth, T, seed, input_slots, hw=HW):
    """x (2T,4,hw,hw), t (2T,) int64, cond dict [uncond; cond] (mirrored in tests/test_long_window_gpu.py and
    tests/test_semidense_cpu.py)"""
    sc = synth.synth_scene(T, (hw, hw), tuple(input_slots), seed=seed)
    x = torch.randn(2 * T, 4, hw, hw, generator=torch.Generator().manual_seed(seed + 1))
    c = {k: torch.cat((sc["uc"][k], sc["cond"][k]), 0) for k in ("crossattn", "concat", "dense_vector")}
    t = torch.full((2 * T,), 979, dtype=torch.int64)
    return x, t, c


@torch.no_grad()
def forward_golden(mg, reval, net, name):
    T, seed = FORWARDS[name]
    slots = input_slots_of(reval, mg.synth, T)
    x, t, c = semidense_inputs(mg.synth, T, seed, slots)
    t0 = time.time()
    y = mg.rmodel.SGMWrapper(net)(x, t, c, num_frames=T)
    dt = time.time() - t0
    print(f"  reference 1.3B forward T={T}, {HW}x{HW}, B={2 * T}, {len(slots)} input slots: {dt:.1f}s", flush=True)
    mg.save(f"{name}_forward", y=y, T=T, h=HW, w=HW, seed=seed, input_slots=np.asarray(slots, dtype=np.int64), ref_seconds=dt,
            ref_threads=torch.get_num_threads())
    size = os.path.getsize(os.path.join(GOLD, f"{name}_forward.npz"))
    assert size <= FILE_LIMIT, f"{name}: {size} bytes is over the limit for a committed file"


def stage_reference(want):
    sys.path.insert(0, HERE)
    import make_goldens as mg  # noqa: E402  (imports the reference + seva.synthetic)
    import make_goldens_next as mn  # noqa: E402  (the reference's seva.eval behind inert UI / IO modules)
    if "plans" in want:
        plans_golden(mn.reval, mg.synth)
    names = [n for n in FORWARDS if n in want]
    if names:
        from make_goldens_headline import full_net
        t0 = time.time()
        net = full_net()
        print(f"  synth 1.3B weights loaded in {time.time() - t0:.1f}s", flush=True)
        for name in names:
            forward_golden(mg, mn.reval, net, name)


# ---------------------------------------------------------------------------------------------------------------- stage 2: parity
def stage_parity(want):
    for p in (ROOT, os.path.join(ROOT, "stable-virtual-camera_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import pytest
    from conftest import load_golden, rel_l2
    from oracle import seva_ref as O
    from seva import synthetic as synth
    from seva.model import Seva, SevaParams
    from test_split_operands_cpu import _emulate

    with torch.device("meta"):
        net = Seva(SevaParams())
    sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 0)
    lines = ["# oracle/make_goldens_semidense.py: the ideal f16 machine (fp32 oracle, GEMM / conv operands rounded to fp16) against the",
             "# stored fp32 reference output, 1.3B synthetic weights, 16 x 16 latent, 32 input slots.  product = the engine's default split",
             "# classes (stem, head, skip_deep) carry their activation operand as hi + lo; floor = every operand plain f16.",
             f"# bound: NET_TOL = {NET_TOL:g}, overall and per latent",
             "# case      T   B    product rel-L2  worst latent   floor rel-L2  worst latent   product < NET_TOL"]
    for name in [n for n in FORWARDS if n in want]:
        g = load_golden(f"{name}_forward")
        T, seed = int(g["T"]), int(g["seed"])
        x, t, c = semidense_inputs(synth, T, seed, g["input_slots"].tolist())
        ref = g["y"]
        fig = []
        for tokens in (("stem", "head", "skip_deep"), ()):
            mp = pytest.MonkeyPatch()
            emu = _emulate(mp, sd, lambda: O.sgm_wrapper_forward(sd, x, t, c, num_frames=T), tokens=tokens)
            fig += [rel_l2(emu, ref), max(rel_l2(emu[i], ref[i]) for i in range(ref.shape[0]))]
        ok = fig[0] < NET_TOL and fig[1] < NET_TOL
        lines.append(f"{name:9s} {T:3d} {2 * T:4d}   {fig[0]:.3e}       {fig[1]:.3e}      {fig[2]:.3e}     {fig[3]:.3e}      {'yes' if ok else 'NO'}")
        print(lines[-1], flush=True)
    with open(LOG, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"  wrote {LOG}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=",".join(["plans"] + list(FORWARDS)))
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--parity-stage", action="store_true", help="(internal) run the second stage in this process")
    args = ap.parse_args()
    want = set(args.only.split(","))
    torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 16)))
    if args.parity_stage:
        return stage_parity(want)
    stage_reference(want)
    if not args.no_parity and want & set(FORWARDS):
        subprocess.run([sys.executable, os.path.abspath(__file__), "--parity-stage", "--only", args.only], check=True)


if __name__ == "__main__":
    main()
