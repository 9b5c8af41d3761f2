"""Semi-dense scenes (nine or more input views): a window length per pass, through the planner and the trajectory driver.

From `num_input_semi_dense` input views on the reference's `infer_prior_stats` rewrites the window lengths (eval.py:344-421): the first
pass is ONE window of all inputs + all anchors (T1 = 27, 41, ... 96), `interp-gt` widens the second pass by the inputs it carries.
`run_one_scene` drives each pass with its own T, cfg and guider (eval.py:1654-1655, 1785-1789, 1929-1933).

a. `pipeline.plan_trajectory` against tests/golden/g15_semidense_plans.json: the reference's own functions in `run_one_scene`'s
   composition (oracle/make_goldens_semidense.py), and against `planner.two_pass_plan`.
b. The driver on tests/fake_ops.py, as test_pipeline_cpu.py does it: 12 inputs, 60 frames; noise draws of the window's own length; two
   gloo ranks, with and without `cfg_split`, equal the single process bit for bit; `cfg` / `guider` pairs reach the right pass.
c. The oracle reproduces the T = 41 golden of the 1.3B network (the pin the other goldens have).
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import GOLD, load_golden, rel_l2
from test_pipeline_cpu import _fake_net, _free_port, _patch_cpu

with open(os.path.join(GOLD, "g15_semidense_plans.json")) as _f:
    G15 = json.load(_f)

# what the issue's table says the reference's rule gives: name -> [T1, T2]
T_PASSES = {"in9_n100": [21, 21], "in9_n330": [27, 21], "in16_n96": [22, 21], "in32_n168": [41, 21], "in12_n120_gt": [21, 33],
            "in32_n168_gt": [41, 53], "in32_n168_T96": [96, 21], "in16_n96_ratio": [23, 21]}


def _plan_of(g):
    from seva import pipeline
    from seva import synthetic as synth
    T = tuple(g["T"]) if isinstance(g["T"], list) else g["T"]
    c2ws = synth.orbit_c2w(g["n"])
    return c2ws, T, pipeline.plan_trajectory(c2ws, g["input_ids"], T=T, chunk_strategy=g["chunk_strategy"],
                                             first_pass_strategy=g["first_pass_strategy"], options=g["options"] or None)


def test_golden_holds_the_cases_of_the_issue():
    assert {k: g["T_passes"] for k, g in G15.items()} == T_PASSES
    assert G15["in32_n168_T96"]["T"] == [96, 21] and G15["in16_n96_ratio"]["options"] == {"num_prior_frames_ratio": 1.2}
    assert all(len(g["input_ids"]) >= 9 for g in G15.values())


@pytest.mark.parametrize("name", list(T_PASSES))
def test_plan_trajectory_reproduces_the_references_semidense_plan(name):
    """Anchors, [T1, T2] and the slot maps of both passes; every window as long as its pass."""
    g = G15[name]
    c2ws, T, tp = _plan_of(g)
    ins, n, prior = g["input_ids"], g["n"], g["prior_inds"]
    T1, T2 = g["T_passes"]
    assert tp.anchor_ids == prior and [tp.T1, tp.T2] == [T1, T2] and tp.T == T1 and tp.input_ids == ins
    order = np.argsort(ins + prior).tolist()
    pool = [(ins + prior)[o] for o in order]
    test = [i for i in range(n) if i not in ins]
    for wins, ref, Tp, src, tgt in ((tp.pass1, g["pass1"], T1, ins + prior, prior), (tp.pass2, g["pass2"], T2, pool, test)):
        assert len(wins) == len(ref["chunks"])
        for w, chunk, ii, isl, ti, ts in zip(wins, ref["chunks"], ref["input_inds"], ref["input_sels"], ref["test_inds"], ref["test_sels"]):
            assert len(chunk) == Tp and len(w.slot_frame) == Tp and len(w.slot_is_input) == Tp
            assert w.source_ids == [src[j] for j in ii] and w.target_ids == [tgt[j] for j in ti] and w.target_slots == list(ts)
            assert set(isl) <= set(w.source_slots)  # (a padded slot that repeats an input is conditioning too)
            # the slot map itself, from the reference's window string: "!007" input 7 of the pool, ">012" target 12, "NULL" padding
            for s, tag in enumerate(chunk):
                if tag.startswith("!"):
                    assert w.slot_is_input[s] and w.slot_frame[s] == src[int(tag[1:])]
                elif tag.startswith(">"):
                    assert not w.slot_is_input[s] and w.slot_frame[s] == tgt[int(tag[1:])]
            assert [w.slot_frame[s] for s in w.target_slots] == w.target_ids
    assert [w.global_index for w in tp.pass1 + tp.pass2] == list(range(len(tp.pass1) + len(tp.pass2)))
    assert sorted(f for w in tp.pass2 for f in w.target_ids) == test


@pytest.mark.parametrize("name", list(T_PASSES))
def test_plan_trajectory_is_two_pass_plans_composition(name):
    from seva import planner as P
    g = G15[name]
    c2ws, T, tp = _plan_of(g)
    plan = P.two_pass_plan(g["n"], g["input_ids"], c2ws, T=T, chunk_strategy=g["chunk_strategy"], options=g["options"] or None,
                           first_pass_strategy=g["first_pass_strategy"])
    assert plan["T"] == [tp.T1, tp.T2] == g["T_passes"] and plan["anchors"] == tp.anchor_ids
    for ours, ref, wins in ((plan["pass1"], g["pass1"], tp.pass1), (plan["pass2"], g["pass2"], tp.pass2)):
        assert list(ours[0]) == ref["chunks"]
        assert [list(ours[1]), list(ours[2]), list(ours[3]), list(ours[4])] == \
               [ref["input_inds"], ref["input_sels"], ref["test_inds"], ref["test_sels"]]
        assert [w.target_slots for w in wins] == [list(ts) for ts in ours[4]]


def test_equal_lengths_leave_the_plan_record_as_it_was():
    """`TrajectoryPlan(T, ...)` positionally, as `plan_views` and earlier callers build it: both passes are T long."""
    from seva import pipeline
    from seva import synthetic as synth
    p = pipeline.TrajectoryPlan(21, [0], [1], [], [], False)
    assert (p.T, p.T1, p.T2) == (21, 21, 21)
    c2ws = synth.orbit_c2w(90)
    pv = pipeline.plan_views(c2ws, list(range(32)), T=90)
    assert (pv.T, pv.T1, pv.T2) == (90, 90, 90) and [len(w.slot_frame) for w in pv.pass1] == [90] and not pv.pass2
    sparse = pipeline.plan_trajectory(synth.orbit_c2w(168), [0, 1, 2], T=21)
    assert (sparse.T, sparse.T1, sparse.T2) == (21, 21, 21)
    assert pipeline.plan_trajectory(synth.orbit_c2w(168), [0, 1, 2], T=(21, 21)).pass2 == sparse.pass2


# ------------------------------------------------------------------------------------------------------------ b. the driver
N_IN, N = 12, 60
SCENES = {"interp": ("interp", None, [21, 21]), "interp-gt": ("interp-gt", None, [21, 33]),
          "interp_prior14": ("interp", {"num_prior_frames": 14}, [26, 21])}


def _scene():
    from seva import synthetic as synth
    g = torch.Generator().manual_seed(3)
    lat = torch.randn(N_IN, 4, 8, 8, generator=g)
    tok = torch.randn(1024, generator=g)
    return synth.orbit_c2w(N), synth.default_K(N), lat, tok / tok.norm()


def _run(scene, group=None, **kw):
    from seva import pipeline
    strategy, options, _ = SCENES[scene]
    c2ws, Ks, lat, tok = _scene()
    return pipeline.run_trajectory(_fake_net, lat, c2ws, Ks, list(range(N_IN)), clip_token=tok, T=21, num_steps=2, seed=23,
                                   device="cpu", group=group, chunk_strategy=strategy, options=options, **kw)


_single = {}


def _single_process(scene, monkeypatch):
    """the single-process run of a scene with what its windows were given, computed once and left unchanged"""
    if scene not in _single:
        from seva import pipeline
        _patch_cpu(monkeypatch)
        seen = []
        inner = pipeline.run_window

        def spy(win, *a, **k):
            seen.append((win.pass_id, win.index, k["noise"].clone(), k["cfg"], k["guider"]))
            return inner(win, *a, **k)
        monkeypatch.setattr(pipeline, "run_window", spy)
        _single[scene] = (_run(scene), seen)
    return _single[scene]


@pytest.mark.parametrize("scene", list(SCENES))
def test_semidense_scene_runs_with_a_window_length_per_pass(scene, monkeypatch):
    res, seen = _single_process(scene, monkeypatch)
    plan, lat = res["plan"], _scene()[2]
    assert [plan.T1, plan.T2] == SCENES[scene][2]
    assert [len(w.slot_frame) for w in plan.pass1] == [plan.T1] * len(plan.pass1)
    assert [len(w.slot_frame) for w in plan.pass2] == [plan.T2] * len(plan.pass2)
    out = res["latents"]
    assert out.shape == (N, 4, 8, 8) and torch.isfinite(out).all()
    assert torch.equal(out[:N_IN], lat)  # the inputs are untouched
    gen = [f for w in plan.pass2 for f in w.target_ids]
    assert sorted(gen) == list(range(N_IN, N))  # every non-input frame is generated (second-pass samples)
    assert all(float(out[f].abs().mean()) > 0 for f in range(N_IN, N))
    # the i-th draw of the ONE CPU stream has the length of window i (reference eval.py:1294-1295)
    wins = plan.pass1 + plan.pass2
    assert [(p, i) for p, i, *_ in seen] == [(w.pass_id, w.index) for w in wins]
    g0 = torch.Generator(device="cpu").manual_seed(23)
    for w, (_, _, noise, _, _) in zip(wins, seen):
        assert torch.equal(noise, torch.randn((len(w.slot_frame), 4, 8, 8), generator=g0))
    assert torch.equal(_run(scene)["latents"], out)


def test_cfg_and_guider_pairs_reach_the_sampler_of_their_pass(monkeypatch):
    """`cfg=(3.0, 2.0)`, `guider=(1, 2)` (reference eval.py:1785-1789, 1929-1933): first-pass windows sample with scale 3 under
    MultiviewCFG, second-pass windows with scale 2 under MultiviewTemporalCFG built with the window's own length."""
    from seva import sampling as S
    _patch_cpu(monkeypatch)
    rec = []

    def hook(sampler):
        g = sampler.guider
        entry = {"guider": type(g).__name__, "num_frames": getattr(g, "num_frames", None), "scales": set()}
        inner = g.frame_scale

        def frame_scale(x, sigma, scale, **kw):
            entry["scales"].add(float(scale))
            return inner(x, sigma, scale, **kw)
        g.frame_scale = frame_scale
        rec.append(entry)

    res = _run("interp-gt", cfg=(3.0, 2.0), guider=(1, 2), sampler_hook=hook)
    plan = res["plan"]
    wins = plan.pass1 + plan.pass2
    assert len(rec) == len(wins) and torch.isfinite(res["latents"]).all()
    for w, r in zip(wins, rec):
        if w.pass_id == 1:
            assert r == {"guider": "MultiviewCFG", "num_frames": None, "scales": {3.0}}
        else:
            assert r == {"guider": "MultiviewTemporalCFG", "num_frames": len(w.slot_frame), "scales": {2.0}}
            assert r["num_frames"] == plan.T2 == 33
    # the pair the other way round: the temporal guider of the first pass is as long as the first-pass window
    rec.clear()
    res = _run("interp_prior14", cfg=2.5, guider=(2, 1), sampler_hook=hook)
    assert [r["guider"] for r in rec] == ["MultiviewTemporalCFG"] + ["MultiviewCFG"] * len(res["plan"].pass2)
    assert rec[0]["num_frames"] == res["plan"].T1 == 26 and all(r["scales"] == {2.5} for r in rec)
    assert isinstance(S.MultiviewTemporalCFG(26, 1.2), S.MultiviewCFG)


def _worker(rank, world, port, q, cfg_split):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _patch_cpu()
    out = {}
    for scene in SCENES:
        res = _run(scene, cfg_split=cfg_split)
        out[scene] = res["latents"].numpy() if "latents" in res else None
    q.put((rank, out))
    dist.destroy_process_group()


@pytest.mark.parametrize("cfg_split", [False, True], ids=["sharded", "cfg_split"])
def test_two_ranks_equal_the_single_process(cfg_split, monkeypatch):
    """Two gloo ranks, windows of two lengths in one trajectory: the anchor all-gather, the second-pass schedule, the gather to rank 0
    and (cfg_split) the pair that splits the CFG batch of the one long first-pass window do not care about the length."""
    from conftest import PKG
    here = os.path.dirname(os.path.abspath(__file__))
    os.environ["PYTHONPATH"] = os.pathsep.join([PKG, here, os.environ.get("PYTHONPATH", "")])
    refs = {scene: _single_process(scene, monkeypatch)[0]["latents"] for scene in SCENES}
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, cfg_split)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for scene, ref in refs.items():
        assert res[1][1][scene] is None  # only rank 0 assembles the trajectory
        got = torch.from_numpy(res[0][1][scene])
        assert torch.equal(got, ref), (scene, float((got - ref).abs().max()))


# ------------------------------------------------------------------------------------------------------------ c. the oracle's pin
def semidense_inputs(T, seed, input_slots, hw=16):
    """Same recipe as oracle/make_goldens_semidense.py:semidense_inputs (x, t, cond [uncond; cond])."""
    from seva import synthetic as synth
    sc = synth.synth_scene(T, (hw, hw), tuple(input_slots), seed=seed)
    x = torch.randn(2 * T, 4, hw, hw, generator=torch.Generator().manual_seed(seed + 1))
    c = {k: torch.cat((sc["uc"][k], sc["cond"][k]), 0) for k in ("crossattn", "concat", "dense_vector")}
    t = torch.full((2 * T,), 979, dtype=torch.int64)
    return x, t, c


@pytest.mark.slow
def test_oracle_reproduces_the_T41_golden():
    """oracle/seva_ref.py against the reference's stored output of one 1.3B call at T = 41, 32 input slots, 16 x 16 latent."""
    from oracle import seva_ref as O
    from seva import synthetic as synth
    from seva.model import Seva, SevaParams
    g = load_golden("g15_T41_forward")
    T, slots = int(g["T"]), g["input_slots"].tolist()
    assert (T, int(g["h"]), int(g["w"])) == (41, 16, 16) and slots == list(range(32)) and g["y"].shape == (82, 4, 16, 16)
    assert slots == G15["in32_n168"]["pass1"]["input_sels"][0]  # the slots the plan of 32 inputs, 168 frames gives them
    with torch.device("meta"):
        net = Seva(SevaParams())
    sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 0)
    x, t, c = semidense_inputs(T, int(g["seed"]), slots)
    torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 16)))
    with torch.no_grad():
        y = O.sgm_wrapper_forward(sd, x, t, c, num_frames=T)
    err = rel_l2(y, g["y"])
    print(f"\noracle vs reference, 1.3B T=41 16x16: rel-L2 {err:.3e}")
    assert err < 5e-5
