"""Two-pass trajectory driver over the hot path (BASELINE config 4: 168-view orbit on 8 GPUs).

Composes what the reference's `run_one_scene` does in its 2-pass branch (seva/eval.py:1631-1959) out of this
package's parts, one process per GPU:

    planner.two_pass_plan            anchors + pass-1 windows + pass-2 windows            (host, every rank, identical)
    pass 1   windows that read only the input views are sharded round-robin over the ranks; a strategy whose windows
             consume earlier windows' outputs (`gt-nearest`, eval.py:1720-1740) runs serially on rank 0
    exchange ONE all-gather of the anchor latents (RCCL over xGMI; <= 20 x 4 x 72 x 72 fp32 = 1.66 MB per rank slot)
    pass 2   windows read only {input views, anchors} (eval.py:1890-1906): independent units, `shard_windows`
    gather   finished window latents to rank 0 (round by round), reassembled in target order, optionally VAE-decoded

CFG-split (`cfg_split=True`): strong scaling of ONE window over a PAIR of ranks -- rank 2j runs the
unconditional half of every CFG batch, rank 2j+1 the conditional half, one 435 KB all-gather per step
(`EulerEDMSampler.cfg_split`).  Used where whole windows cannot fill the ranks: the serial first pass (pair 0) and the
leftover second-pass round (10 windows on 8 GPUs: 8 whole windows, then the last 2 on pairs (0,1), (2,3)):
168 views on 8 GPUs = 0.5 + 1 + 0.5 window times instead of 1 + 2 (ceiling 5.5x instead of 3.7x).  Bitwise the same trajectory.

Hand-off between the passes: the reference carries the anchors across the pass boundary as decoded RGB and re-encodes
them per window (eval.py:1820-1829, 1246).  Here the default hand-off is the anchor LATENT itself (`handoff="latent"`:
no decode -> encode round trip, 1.66 MB instead of 40 MB on the wire); `handoff="rgb"` reproduces the reference's
round trip through `AutoEncoder.decode` / `.encode` when an `ae` is given.

Window lengths: a sparse scene runs every window at T.  From nine input views on (`num_input_semi_dense`) the reference's
`infer_prior_stats` gives each pass its own length (eval.py:344-421: the first pass is ONE window of all inputs + all anchors,
`interp-gt` widens the second pass by the inputs it carries) and `run_one_scene` drives each pass with its own T, cfg and guider
(eval.py:1654-1655, 1785-1789, 1929-1933); so do `plan_trajectory` (`TrajectoryPlan.T1` / `.T2`) and `run_trajectory`, whose `T`,
`cfg` and `guider` take one value or a (first pass, second pass) pair.  A window is `len(win.slot_frame)` views long; nothing
else in the driver reads a length.

Randomness under sharding (SURVEY §8e last bullet; reference eval.py:1294-1295, 1450): the initial noise of window i is
the i-th `torch.randn((len(window),4,h,w))` draw of ONE CPU stream seeded once per scene -- every rank draws the whole sequence
in plan order and keeps its own windows'.  The per-step device noise (`randn_like`, sampling.py:359) comes from a
generator owned by the window (seed = scene seed, window index), so a window's result does not depend on which rank
runs it or on what ran before it: a sharded run equals the sequential run bit for bit (tested on gloo, world size 2).

CLIP token: `clip_token` (one 1024-d token for every window), `clip_fn(window_source_ids) -> (1024,)`, or -- the reference's
own rule (eval.py:1248: mean CLIP embedding of the window's conditioning views) -- `conditioner=` + `input_rgb=` with
`handoff="rgb"` and an `ae`: the anchors are then decoded once after pass 1, every window's token is
`conditioner(rgb of its conditioning frames).mean(0)` and the anchors re-enter pass 2 through `ae.encode`, as in the reference.

One pass (`plan_views` / `run_views`, `run_scene(use_traj_prior=False)`): the reference's evaluation mode (eval.py:1472-1629,
tasks `img2img` / `img2vid`) -- the first-pass half of the plan over EVERY non-input frame, no second pass; the same driver
runs it.  `run_scene(targets=...)` scores the generated frames against held-out pictures (`seva.metrics`: PSNR / SSIM, and LPIPS
with `lpips=`).
"""

from __future__ import annotations

import time
from dataclasses import dataclass, field
from typing import Callable, Sequence

import numpy as np
import torch
import torch.distributed as dist

from . import conditioning, planner
from . import sampling as S

DEPENDENT_FIRST_PASS = ("gt-nearest", "gt-ltr")  # windows consume earlier windows' outputs (eval.py:530-616)


@dataclass
class Window:
    pass_id: int                  # 1 or 2
    index: int                    # position inside its pass
    global_index: int             # position in the scene-wide draw order of the initial noise
    source_ids: list[int]         # trajectory frame ids of the conditioning frames (inputs, earlier outputs, anchors)
    source_slots: list[int]
    target_ids: list[int]         # trajectory frame ids this window generates
    target_slots: list[int]
    slot_frame: list[int] = field(default_factory=list)   # per slot: trajectory frame id (padding repeats a frame)
    slot_is_input: list[bool] = field(default_factory=list)


@dataclass
class TrajectoryPlan:
    T: int
    input_ids: list[int]
    anchor_ids: list[int]
    pass1: list[Window]
    pass2: list[Window]
    pass1_serial: bool
    T1: int | None = None         # window length of the first pass (None: `T`)
    T2: int | None = None         # window length of the second pass (None: `T`)

    def __post_init__(self):
        self.T1 = self.T if self.T1 is None else int(self.T1)
        self.T2 = self.T if self.T2 is None else int(self.T2)


def _windows(pass_id, base, T, chunks, src_pool, tgt_pool, padding_mode="last"):
    _, ins, in_slots, tes, te_slots = chunks
    out = []
    for i, (ci, cs, ti, ts) in enumerate(zip(ins, in_slots, tes, te_slots)):
        cs2, ts2, in_map, te_map = planner.pad_indices(list(cs), list(ts), T=T, padding_mode=padding_mode)
        slot_frame, slot_in = [], []
        for s in range(T):
            if in_map[s] != -1:
                slot_frame.append(src_pool[ci[in_map[s]]])
                slot_in.append(True)
            else:
                slot_frame.append(tgt_pool[ti[te_map[s]]])
                slot_in.append(False)
        out.append(Window(pass_id, i, base + i, [src_pool[j] for j in ci], list(cs), [tgt_pool[j] for j in ti], list(ts),
                          slot_frame, slot_in))
        # a padded slot that repeats an INPUT frame is conditioning too (reference: curr_input_sels after pad_indices)
        out[-1].source_slots = [s for s in range(T) if slot_in[s]]
    return out


def _input_conditioned_windows(c2ws, ins, targets, T, opts, task, strategy):
    """Windows that generate the frames `targets` from the input views `ins` (the two-pass mode's first pass over the
    anchors, the one-pass mode's only pass over every non-input frame) -> (windows, serial)."""
    p1 = planner.chunk_input_and_test(T, c2ws[ins], c2ws[targets], [float(i) for i in ins], [float(a) for a in targets],
                                      opts, task=task, chunk_strategy=strategy, gt_input_inds=list(range(len(ins))))
    serial = strategy in DEPENDENT_FIRST_PASS
    # source pool: the inputs, then (dependent strategies) the targets in the order they are generated
    pool1 = list(ins)
    if serial:
        for ti in p1[3]:
            pool1.extend(targets[j] for j in ti)
    return _windows(1, 0, T, p1, pool1, targets, opts.get("t_padding_mode", "last")), serial


def plan_views(c2ws: torch.Tensor, input_ids: Sequence[int], T: int = 21, chunk_strategy: str = "gt",
               options: dict | None = None, task: str = "img2img") -> TrajectoryPlan:
    """One-pass plan (the reference's `use_traj_prior=False` branch, eval.py:1472-1629, the mode of its evaluation tasks
    `img2img` / `img2vid`): every non-input frame is a target of ONE pass of windows conditioned on the input views
    (`chunk_strategy`, default "gt"; dependent strategies also read earlier windows' outputs, in generation order).  In
    the plan's terms every non-input frame stands in the anchors' place and `pass2` is empty, which `run_trajectory`
    drives as it is: independent windows sharded round-robin over the ranks, dependent ones serial on rank 0."""
    ins = [int(i) for i in input_ids]
    opts = {"sampler_verbose": False, **(options or {}), "chunk_strategy": chunk_strategy}
    targets = [i for i in range(c2ws.shape[0]) if i not in set(ins)]
    w1, serial = _input_conditioned_windows(c2ws, ins, targets, T, opts, task, chunk_strategy)
    return TrajectoryPlan(T, ins, targets, w1, [], serial)


def plan_trajectory(c2ws: torch.Tensor, input_ids: Sequence[int], T: int | Sequence[int] = 21, chunk_strategy: str = "interp",
                    first_pass_strategy: str = "gt-nearest", options: dict | None = None,
                    task: str = "img2trajvid", refine_anchors: bool = True,
                    anchor_ids: Sequence[int] | None = None) -> TrajectoryPlan:
    """Anchors + windows of both passes for one trajectory; frame ids index `c2ws` (inputs first, like the reference's
    `input_indices` convention in run_one_scene).

    Defaults are the reference's (eval.py:1656 `chunk_strategy_first_pass` = "gt-nearest"; eval.py:1459 + 1869-1885: the
    second pass targets EVERY non-input frame, so the anchors -- which the `interp` chunker places as the first target of
    the range they open -- are generated again in pass 2 and the trajectory's anchor frames are second-pass samples;
    golden: tests/golden/g10_two_pass_plans.json).  `refine_anchors=False` is this package's cheaper variant: the second
    pass skips the anchors and their final latents are the first-pass samples (one target slot more per range).

    `T`: one window length or a pair (T1, T2).  From `num_input_semi_dense` (9) input views on, `infer_prior_stats` rewrites
    the lengths as the reference does (eval.py:344-421): the first pass becomes ONE window of all inputs + all anchors, and
    `interp-gt` widens the second pass by the input views it carries (golden: tests/golden/g15_semidense_plans.json).  The plan
    records both (`T1`, `T2`); `T` is the first-pass length.  `options` carries `num_prior_frames_ratio`, `num_prior_frames`
    and `num_input_semi_dense`.

    `anchor_ids`: None (the default) lets `infer_prior_inds` choose the anchors; a list of frame ids takes that choice's place (the
    reference's callers hand `run_one_scene` their own anchors: demo.py:231-256 spreads them over the targets with a rounding rule
    of its own; `seva.scenes` is the caller here).  The ids must lie in the trajectory, and must not be input views; they are used in
    ascending order, like `infer_prior_inds`' own, and an id given twice (the rounding rule repeats ids where it asks for more
    anchors than there are targets) counts once.

    Limit: a window length that leaves fewer than two free target slots (T < inputs + 2; under `interp-gt`, T < inputs + 4) makes the
    chunkers loop without end ("Known limit").  The window lengths still follow `infer_prior_stats`."""
    n = c2ws.shape[0]
    ins = [int(i) for i in input_ids]
    opts = {"sampler_verbose": False, **(options or {}), "chunk_strategy": chunk_strategy}
    T = [int(t) for t in T] if isinstance(T, (list, tuple)) else int(T)
    vd = {"T": T, "options": opts}
    n_prior = planner.infer_prior_stats(T, len(ins), n - len(ins), vd)
    T1, T2 = (int(t) for t in S.per_pass(vd["T"]))
    if anchor_ids is None:
        anchors = [int(v) for v in planner.infer_prior_inds(c2ws, n_prior, ins, opts)]
    else:
        if any(int(v) != v for v in anchor_ids):
            raise ValueError(f"anchor_ids: integer frame ids, not {list(anchor_ids)!r}")
        anchors = sorted({int(v) for v in anchor_ids})
        bad = [a for a in anchors if not 0 <= a < n]
        if not anchors or bad:
            raise ValueError(f"anchor_ids: {'an empty list' if not anchors else f'{bad} outside the {n} frames of the trajectory'}")
        if set(anchors) & set(ins):
            raise ValueError(f"anchor_ids: {sorted(set(anchors) & set(ins))} are input views")
    w1, serial = _input_conditioned_windows(c2ws, ins, anchors, T1, opts, task, first_pass_strategy)
    order = np.argsort(ins + anchors).tolist()
    pool2 = [(ins + anchors)[o] for o in order]
    skip = set(ins) if refine_anchors else set(ins) | set(anchors)
    rest = [i for i in range(n) if i not in skip]
    p2 = planner.chunk_input_and_test(T2, c2ws[pool2], c2ws[rest], [float(i) for i in pool2], [float(r) for r in rest],
                                      opts, task=task, chunk_strategy=chunk_strategy,
                                      gt_input_inds=[order.index(i) for i in range(len(ins))])
    w2 = _windows(2, len(w1), T2, p2, pool2, rest)
    return TrajectoryPlan(T1, ins, anchors, w1, w2, serial, T1, T2)


def _rank_world(group=None):
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


def _all_gather_padded(local: torch.Tensor, count: int, max_count: int, group=None) -> list[torch.Tensor]:
    """All-gather of per-rank tensors with different leading sizes: each rank pads to `max_count` rows."""
    rank, world = _rank_world(group)
    if world == 1:
        return [local[:count]]
    buf = torch.zeros((max_count,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    buf[:count] = local[:count]
    out = torch.empty((world * max_count,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(out, buf.contiguous(), group=group)
    return list(out.view(world, max_count, *local.shape[1:]).unbind(0))


_pair_groups: dict = {}


def _now(device) -> float:
    """The drivers' one clock (`run_trajectory(timers=...)`: stages and windows): wall time after the device has drained."""
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    return time.perf_counter()


def cfg_pair_groups(group=None) -> list:
    """Two-rank process groups (0,1), (2,3), ... of `group` (default: the world), created once per process: every rank
    calls this (new_group is collective) and gets the same list; entry j is the group of ranks 2j and 2j+1."""
    rank, world = _rank_world(group)
    key = (id(group), world)
    if key not in _pair_groups:
        ranks = list(range(world)) if group is None else dist.get_process_group_ranks(group)
        _pair_groups[key] = [dist.new_group([ranks[2 * j], ranks[2 * j + 1]]) for j in range(world // 2)]
    return _pair_groups[key]


def second_pass_schedule(n_windows: int, world: int, cfg_split: bool) -> list[list[tuple]]:
    """Rounds of (window index, ranks) for the second pass.  Whole-window rounds: window r*world + q on rank q.  With
    `cfg_split`, a last round of L <= world/2 leftover windows runs window j on the pair (2j, 2j+1)."""
    rounds, i = [], 0
    while i < n_windows:
        left = n_windows - i
        if cfg_split and world >= 2 and left <= world // 2:
            rounds.append([(i + j, (2 * j, 2 * j + 1)) for j in range(left)])
            i += left
        else:
            k = min(left, world)
            rounds.append([(i + q, (q,)) for q in range(k)])
            i += k
    return rounds


def run_window(win: Window, latents_of: dict, denoise_net: Callable, c2ws, Ks, *, hw, num_steps, cfg, cfg_min, guider,
               camera_scale, noise: torch.Tensor, step_seed: int, clip_token: torch.Tensor, device,
               sampler_hook: Callable | None = None, cfg_split: tuple | None = None,
               solver: str | None = None, cache_interval: int | None = None, cache_levels: int | None = 1,
               guidance_interval=None, guidance_rescale: float | None = None) -> torch.Tensor:
    """One window = the reference's get_value_dict + do_sample (eval.py:1152-1321) on this package's parts.
    `latents_of[frame_id]` -> (4,h,w) latent of every conditioning frame.  Returns the (T,4,h,w) sample.
    The sampler options go to the window's `EulerEDMSampler` as they are, and its docstring describes them: `solver` ("euler",
    "dpmpp2m"), `cache_interval` / `cache_levels` (the opt-in reuse of deep UNet features across steps), `guidance_interval` =
    (sigma_lo, sigma_hi) / `guidance_rescale` = phi (the opt-in guidance controls).  None reads the option's SEVA_* variable
    (`sampling.resolve_options`); everything is off by default."""
    options = dict(solver=solver, cache_interval=cache_interval, cache_levels=cache_levels, guidance_interval=guidance_interval,
                   guidance_rescale=guidance_rescale)
    T = len(win.slot_frame)
    h, w = hw
    frames = win.slot_frame
    mask = torch.tensor(win.slot_is_input, dtype=torch.bool)
    in_slots = [s for s in range(T) if win.slot_is_input[s]]
    vd = conditioning.get_value_dict((h * 8, w * 8), in_slots, c2ws[frames][:, :3], Ks[frames].clone(), c2ws,
                                     camera_scale, device=device)
    lat = torch.stack([latents_of[frames[s]] for s in in_slots]).to(device)
    cond, uc = conditioning.assemble_cond(lat, clip_token, mask, vd["plucker_coordinate"])
    disc = S.DDPMDiscretization()
    den = S.DiscreteDenoiser(disc, num_idx=1000, device=device)
    g = [S.VanillaCFG(), S.MultiviewCFG(cfg_min), S.MultiviewTemporalCFG(T, cfg_min)][guider]
    sampler = S.EulerEDMSampler(disc, g, num_steps=num_steps, verbose=False, device=device, s_churn=0.0, **options)
    gen = torch.Generator(device=device)
    gen.manual_seed(int(step_seed))
    sampler.noise_fn = lambda x: torch.randn(x.shape, generator=gen, device=x.device, dtype=x.dtype)
    sampler.cfg_split = cfg_split  # (two-rank group, half): both ranks draw the same per-step noise from `step_seed`
    if sampler_hook is not None:
        sampler_hook(sampler)
    kw = {} if guider == 0 else dict(c2w=vd["c2w"].to(device), K=Ks[frames].to(device), input_frame_mask=mask.to(device))
    return sampler(lambda x, s, c: den(denoise_net, x, s, c, num_frames=T), noise.to(device).clone(), scale=cfg,
                   cond=cond, uc=uc, verbose=False, **kw)


@dataclass
class _Trajectory:
    """What the stages of `run_trajectory` share: one record per call, alike on every rank but for `rank`."""
    plan: TrajectoryPlan
    net: Callable                 # `denoise_net`
    c2ws: torch.Tensor
    Ks: torch.Tensor
    hw: tuple                     # latent (h, w)
    seed: int
    device: torch.device
    group: object
    rank: int
    world: int
    timers: dict | None
    ae: object
    rgb_handoff: bool             # the hand-off goes decode -> encode through `ae`
    conditioner: Callable | None
    token: Callable               # a window's source ids -> its CLIP token
    rgb_of: dict                  # frame id -> RGB, kept under `conditioner=` for the windows' tokens
    latents_of: dict              # frame id -> the (4,h,w) latent that later windows condition on
    noises: list                  # initial noise per window, in draw order (`Window.global_index`)
    passes: tuple                 # per pass: the `run_window` keywords of its windows (cfg, guider, sampler options)
    common: dict                  # the `run_window` keywords of every window
    pairs: list = field(default_factory=list)  # `cfg_pair_groups` under cfg_split

    @property
    def split1(self) -> bool:
        """serial strategies (and, under cfg_split, every one-window first pass): pair 0 = ranks (0, 1) splits the CFG batch of each window"""
        return bool(self.pairs) and (self.plan.pass1_serial or len(self.plan.pass1) == 1)

    @property
    def keep_own(self) -> bool:
        """one pass + RGB hand-off: a frame's OUTPUT is its own sample (the reference decodes it directly, `decode_output`); only
        later windows see the re-encoded latent.  (Two passes keep the handed-off latent for anchors the second pass does not
        regenerate.)"""
        return self.rgb_handoff and not self.plan.pass2

    def mark(self, name):
        if self.timers is not None:
            self.timers[name] = _now(self.device)


def _token_rule(plan, device, clip_token, clip_fn, conditioner, input_rgb, ae, handoff):
    """-> (a window's source ids -> its CLIP token, the `rgb_of` the rule reads: empty without a `conditioner`)"""
    if conditioner is None:
        assert clip_fn is not None or clip_token is not None, "a CLIP token (clip_token / clip_fn / conditioner) is required"
        return ((lambda ids: clip_token) if clip_fn is None else clip_fn), {}
    # the reference's rule (eval.py:1248): token of a window = mean CLIP embedding of its conditioning views' RGB
    assert input_rgb is not None and ae is not None and handoff == "rgb", \
        "conditioner= needs input_rgb=, ae= and handoff='rgb' (anchor RGB comes from the VAE decode between the passes)"
    rgb_of = {fid: input_rgb[i].to(device) for i, fid in enumerate(plan.input_ids)}
    return (lambda ids: conditioner(torch.stack([rgb_of[f] for f in ids])).mean(0)), rgb_of


def _draw_noises(plan, seed, hw):
    """initial noise: ONE CPU stream, seeded once per scene, drawn in plan order for EVERY window (eval.py:1294-1295,1450)"""
    g0 = torch.Generator(device="cpu")
    g0.manual_seed(seed)
    return [torch.randn((len(win.slot_frame), 4, *hw), generator=g0) for win in plan.pass1 + plan.pass2]


def first_pass_owner(plan: TrajectoryPlan, i: int, world: int, split1: bool) -> int:
    """The rank that owns first-pass window i, that is, publishes its targets in the anchor exchange.  Rank 0 where the pass runs in
    one place -- one process, a serial strategy, or `split1` (rank 1 of pair 0 runs every window too and holds the same bits, but
    does not publish) -- and round-robin otherwise, as `distributed.shard_windows` deals windows."""
    return 0 if (world == 1 or plan.pass1_serial or split1) else i % world


def _run_one(run: _Trajectory, win: Window, ranks: tuple) -> torch.Tensor:
    """`run_window` of `win` on this rank, with the window's own noise, step seed, token and pass settings; `ranks` = (q,): the whole
    window, (2j, 2j+1): this rank's half of every CFG batch in pair j.  Appends (pass, index, seconds) to `timers["windows"]`."""
    t0 = _now(run.device) if run.timers is not None else 0.0
    # step seed = the per-window device stream: independent of rank and of execution order
    z = run_window(win, run.latents_of, run.net, run.c2ws, run.Ks, noise=run.noises[win.global_index],
                   step_seed=(run.seed * 1000003 + 7919 * (win.global_index + 1)) & 0x7FFFFFFFFFFF,
                   clip_token=run.token(win.source_ids),
                   cfg_split=(run.pairs[ranks[0] // 2], ranks.index(run.rank)) if len(ranks) == 2 else None,
                   **run.passes[win.pass_id - 1], **run.common)
    if run.timers is not None:
        run.timers.setdefault("windows", []).append((win.pass_id, win.index, _now(run.device) - t0))
    return z


def _hand_off(run: _Trajectory, z, fids):
    """(k,4,h,w) generated latents -> what the next window conditions on"""
    if not run.rgb_handoff:
        return z
    rgb = run.ae.decode(z)
    if run.conditioner is not None:
        run.rgb_of.update(zip(fids, rgb))
    return run.ae.encode(rgb)


def _first_pass(run: _Trajectory) -> tuple:
    """This rank's first-pass windows -> (handed-off latents, own samples under `keep_own`) of the targets it publishes."""
    plan, split1 = run.plan, run.split1
    pub_lat, pub_own = [], []
    for i, win in enumerate(plan.pass1):
        owner = first_pass_owner(plan, i, run.world, split1)
        ranks = (0, 1) if split1 else (owner,)
        if run.rank not in ranks:
            continue
        own = _run_one(run, win, ranks)[win.target_slots]
        handed = _hand_off(run, own, win.target_ids)
        run.latents_of.update(zip(win.target_ids, handed))  # a dependent strategy's next window on this rank may read it
        if run.rank == owner:
            pub_lat.extend(handed)
            if run.keep_own:
                pub_own.extend(own)
    return pub_lat, pub_own


def _exchange_anchors(run: _Trajectory, pub_lat: list, pub_own: list) -> dict:
    """ONE all-gather of the first-pass targets into `latents_of` on every rank; under `keep_own` a second one, of the own samples
    -> {frame id: own sample} (else {})."""
    plan, world = run.plan, run.world
    owner_ids = [[] for _ in range(world)]
    for i, win in enumerate(plan.pass1):
        owner_ids[first_pass_owner(plan, i, world, run.split1)].extend(win.target_ids)
    counts = [len(ids) for ids in owner_ids]

    def gathered(rows):
        local = torch.stack(rows) if rows else torch.zeros((0, 4, *run.hw), device=run.device)
        parts = _all_gather_padded(local.to(device=run.device, dtype=torch.float32), counts[run.rank], max(max(counts), 1), run.group)
        return {fid: parts[r][j] for r in range(world) for j, fid in enumerate(owner_ids[r])}

    run.latents_of.update(gathered(pub_lat))
    own_of = gathered(pub_own) if run.keep_own else {}
    if run.conditioner is not None and plan.pass2:
        # ranks that did not generate an anchor need its RGB for the CLIP token: decode locally (1.66 MB of latents travelled, not
        # 40 MB of RGB)
        for fid in plan.anchor_ids:
            if fid not in run.rgb_of:
                run.rgb_of[fid] = run.ae.decode(run.latents_of[fid][None])[0]
    return own_of


def _second_pass(run: _Trajectory) -> tuple:
    """Independent windows, sharded by `second_pass_schedule` -> (the schedule, {window index: sample} of this rank's windows)."""
    sched = second_pass_schedule(len(run.plan.pass2), run.world, bool(run.pairs))
    outs = {}
    for rnd in sched:
        for i, ranks in rnd:
            if run.rank in ranks:
                outs[i] = _run_one(run, run.plan.pass2[i], ranks)
    return sched, outs


def _gather(run: _Trajectory, sched: list, outs: dict) -> dict:
    """The second-pass samples to rank 0, one `dist.gather` per round -> {window index: sample} there."""
    rank, world = run.rank, run.world
    collected = {}
    for rnd in sched:
        sender = {ranks[0]: i for i, ranks in rnd}  # a pair's even rank sends (both hold the same bits)
        mine = outs.get(sender[rank]) if rank in sender else None
        if world == 1:
            if mine is not None:
                collected[sender[rank]] = mine
            continue
        send = mine if mine is not None else torch.zeros((run.plan.T2, 4, *run.hw), device=run.device)
        bufs = [torch.empty_like(send) for _ in range(world)] if rank == 0 else None
        dist.gather(send.contiguous(), bufs, dst=0, group=run.group)
        if rank == 0:
            for rr, i in sender.items():
                collected[i] = bufs[rr]
    return collected


def _assemble(run: _Trajectory, collected: dict, own_of: dict) -> dict:
    """Rank 0: the frames in target order, optionally VAE-decoded -> the result of `run_trajectory`."""
    plan, latents_of = run.plan, run.latents_of
    n = run.c2ws.shape[0]
    final = torch.zeros((n, 4, *run.hw), device=run.device)
    filled = torch.zeros(n, dtype=torch.bool)
    for fid in plan.input_ids + plan.anchor_ids:  # (anchors: first-pass samples, overwritten below when pass 2 regenerates them)
        final[fid] = own_of.get(fid, latents_of[fid])
        filled[fid] = True
    for i, win in enumerate(plan.pass2):
        z = collected[i]
        for fid, slot in zip(win.target_ids, win.target_slots):
            final[fid] = z[slot]
            filled[fid] = True
    assert bool(filled.all()), f"frames never generated: {torch.nonzero(~filled).flatten().tolist()}"
    # "anchor_latents": what pass 2 conditioned on (first-pass samples after the hand-off), whether or not pass 2 regenerated them
    res = {"latents": final, "frame_ids": list(range(n)), "plan": plan,
           "anchor_latents": {fid: latents_of[fid] for fid in plan.anchor_ids}}
    if run.ae is not None:
        res["rgb"] = run.ae.decode(final)
        run.mark("decode")
    return res


def run_trajectory(denoise_net: Callable, input_latents: torch.Tensor, c2ws: torch.Tensor, Ks: torch.Tensor,
                   input_ids: Sequence[int], *, clip_token: torch.Tensor | None = None, clip_fn: Callable | None = None,
                   T: int | Sequence[int] = 21, num_steps: int = 50, cfg: float | Sequence[float] = 2.0, cfg_min: float = 1.2,
                   guider: int | Sequence[int] = 1,
                   camera_scale: float = 2.0, seed: int = 23, chunk_strategy: str = "interp", options: dict | None = None,
                   first_pass_strategy: str = "gt-nearest", refine_anchors: bool = True, device=None, group=None, ae=None,
                   handoff: str = "latent",
                   plan: TrajectoryPlan | None = None, timers: dict | None = None,
                   sampler_hook: Callable | None = None, conditioner: Callable | None = None,
                   input_rgb: torch.Tensor | None = None, cfg_split: bool = False, solver: str | None = None,
                   cache_interval=None, cache_levels=1, guidance_interval=None, guidance_rescale=None,
                   anchor_ids: Sequence[int] | None = None) -> dict:
    """Generate every non-input frame of a trajectory.  `denoise_net(x, t, cond, num_frames=T)` is the network call
    (`SGMWrapper(model)`); `input_latents` (n_in,4,h,w) are the VAE-encoded input views (x 0.18215), frame ids
    `input_ids` index `c2ws` (n,4,4) / `Ks` (n,3,3).  Returns, on rank 0, {"latents": (n,4,h,w) in frame order,
    "frame_ids", "plan", "anchor_latents" (first-pass anchors as pass 2 saw them), ["rgb"]}; other ranks get {"plan"} only.
    The sampler options (`run_window` lists them) go to every window's sampler.  `solver` is one value; each of the others is one
    value or a (first pass, second pass) pair, by the rule of `sampling.per_pass_options` (for `guidance_interval` a pair is a
    2-tuple whose elements are themselves (lo, hi) tuples or None, and a 2-tuple of numbers is one interval for both passes).
    `T`, `cfg` and `guider` each take one value or a (first pass, second pass) pair, as the reference's `--T 96,21` /
    `cfg 3,2` do (eval.py:1785-1789, 1929-1933); `options` goes to the planner (`num_prior_frames_ratio`, ...).  A window
    is as long as its pass of the plan says (`plan.T1` / `plan.T2`): its noise draw, its guider and its network call.
    `anchor_ids` goes to `plan_trajectory` (None: the planner's own anchors); with a ready `plan=` it is not read.
    `timers`: a dictionary that receives the wall clock at the end of each stage below ("start", "pass1", "exchange", "pass2",
    "gather", "decode") and "windows" = [(pass, index, seconds)] of this rank's windows."""
    sampler_options = dict(solver=solver, cache_interval=cache_interval, cache_levels=cache_levels,
                           guidance_interval=guidance_interval, guidance_rescale=guidance_rescale)
    rank, world = _rank_world(group)
    device = torch.device(device) if device is not None else input_latents.device
    hw = tuple(input_latents.shape[-2:])
    plan = plan or plan_trajectory(c2ws, input_ids, T, chunk_strategy, first_pass_strategy, options,
                                   refine_anchors=refine_anchors, anchor_ids=anchor_ids)
    passes = tuple({"cfg": c, "guider": g, **o}
                   for c, g, o in zip(S.per_pass(cfg), S.per_pass(guider), S.per_pass_options(**sampler_options)))
    token, rgb_of = _token_rule(plan, device, clip_token, clip_fn, conditioner, input_rgb, ae, handoff)
    run = _Trajectory(plan=plan, net=denoise_net, c2ws=c2ws, Ks=Ks, hw=hw, seed=int(seed), device=device, group=group, rank=rank,
                      world=world, timers=timers, ae=ae, rgb_handoff=handoff == "rgb" and ae is not None, conditioner=conditioner,
                      token=token, rgb_of=rgb_of, noises=_draw_noises(plan, int(seed), hw), passes=passes,
                      latents_of={fid: input_latents[i].to(device) for i, fid in enumerate(plan.input_ids)},
                      common=dict(hw=hw, num_steps=num_steps, cfg_min=cfg_min, camera_scale=camera_scale, device=device,
                                  sampler_hook=sampler_hook))
    run.mark("start")
    if cfg_split and world >= 2:
        run.pairs = cfg_pair_groups(group)
    published = _first_pass(run)
    run.mark("pass1")
    own_of = _exchange_anchors(run, *published)
    run.mark("exchange")
    sched, outs = _second_pass(run)
    run.mark("pass2")
    collected = _gather(run, sched, outs)
    run.mark("gather")
    return _assemble(run, collected, own_of) if rank == 0 else {"plan": plan}


def run_views(denoise_net: Callable, input_latents: torch.Tensor, c2ws: torch.Tensor, Ks: torch.Tensor,
              input_ids: Sequence[int], *, T: int = 21, chunk_strategy: str = "gt", options: dict | None = None,
              task: str = "img2img", **run_trajectory_kwargs) -> dict:
    """One-pass generation of every non-input frame: `run_trajectory` over `plan_views(...)`; every other argument (the sampler
    options, `solver` to `guidance_rescale`, among them) and the result are `run_trajectory`'s ("anchor_latents": every generated
    frame as later windows saw it)."""
    plan = plan_views(c2ws, input_ids, T, chunk_strategy, options, task)
    return run_trajectory(denoise_net, input_latents, c2ws, Ks, input_ids, T=T, plan=plan, **run_trajectory_kwargs)


def run_scene(denoise_net: Callable, ae, images: Sequence, c2ws: torch.Tensor, Ks: torch.Tensor, input_ids: Sequence[int], *,
              size=(576, 576), conditioner: Callable | None = None, clip_token: torch.Tensor | None = None,
              use_traj_prior: bool = True, targets: dict | None = None, lpips=None, **run_trajectory_kwargs) -> dict:
    """Pictures + cameras in, uint8 frames out: `frames.load_img_and_K` per input picture (a path, a uint8 (h,w,3|4) array
    or tensor; covered and cropped to `size` = (W, H)), `ae.encode`, `run_trajectory`, `ae.decode`, `frames.to_uint8`.
    `Ks` (n,3,3) as `run_trajectory` takes them (normalised); the input views' rows are replaced by the intrinsics of the
    cropped pictures.  With a `conditioner` the loaded pictures are its `input_rgb` and the hand-off goes through RGB, as
    `run_trajectory` requires.  A composition only: on rank 0 the result of `run_trajectory` (with "rgb") plus "frames"
    (n,H,W,3) uint8 and "Ks" (n_in,3,3), the adjusted intrinsics of the input views in pixels of the frames.
    `use_traj_prior=False`: the reference's one-pass evaluation mode (`run_views`; `chunk_strategy` then defaults to "gt",
    `options` / `task` go to `plan_views`).  `targets` = {frame id: picture}: held-out pictures, loaded exactly like the inputs
    and scored against the generated frames of those ids (`metrics.compare` on the uint8 frames) -> on rank 0
    "metrics" = {"frame_ids", "sse", "psnr", "ssim"}; in either mode.  `lpips` (a `metrics.LPIPS` on the device; frames of at
    least 32 x 32) adds "lpips" to that table: the complete score table without the frames leaving the card.
    The sampler options (`run_window` lists them, `solver=` to `guidance_rescale=`) travel to `run_trajectory`; with
    `use_traj_prior=False` and `targets=` this is the call that measures what one of them does to picture quality."""
    from . import frames
    device = torch.device(run_trajectory_kwargs.pop("device", None) or "cuda")
    ids = [int(i) for i in input_ids]
    assert len(images) == len(ids), "one picture per input view"
    rgb, K_px = [], []
    Ks = Ks.clone()
    for img, fid in zip(images, ids):
        x, K = frames.load_img_and_K(img, size, K=Ks[fid], device=device)
        H, W = x.shape[-2:]
        rgb.append(x)
        K_px.append(K)
        Ks[fid] = K / K.new_tensor([W, H, 1.0])[:, None]  # back to normalised intrinsics (eval.py:1400-1401)
    input_rgb = torch.cat(rgb)
    kw = dict(run_trajectory_kwargs)
    if conditioner is not None:
        kw.update(conditioner=conditioner, input_rgb=input_rgb)
        kw.setdefault("handoff", "rgb")
    run = run_trajectory if use_traj_prior else run_views
    res = run(denoise_net, ae.encode(input_rgb), c2ws, Ks, ids, clip_token=clip_token, device=device, ae=ae, **kw)
    if "rgb" in res:  # rank 0
        res["frames"] = frames.to_uint8(res["rgb"])
        res["Ks"] = torch.stack(K_px)
        if targets:
            from . import metrics
            tids = sorted(int(f) for f in targets)
            want = torch.cat([frames.to_uint8(frames.load_img_and_K(targets[f], size, device=device)[0]) for f in tids])
            m = metrics.compare(res["frames"][tids], want, lpips=lpips)
            res["metrics"] = {"frame_ids": tids, "sse": m["sse"], "psnr": m["psnr"], "ssim": m["ssim"]}
            if lpips is not None:
                res["metrics"]["lpips"] = m["lpips"]
    return res
