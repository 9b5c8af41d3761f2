"""`seva.sampling` -- drop-in operator API of the reference sampler (seva/sampling.py) on MI355X.

Same classes, constructor arguments, attributes and call signatures as the reference
(SURVEY.md §8b): `DDPMDiscretization`, `DiscreteDenoiser`, `VanillaCFG`, `MultiviewCFG`,
`MultiviewTemporalCFG`, `EulerEDMSampler` (+ the helpers they are built from).

Division of labour
  * Everything that touches a latent-sized tensor ((T,4,h,w) and up) -- replace-blend, c_in
    scaling, c_out/c_skip combine, noise injection, CFG combine, Euler update -- is a HIP kernel
    of libseva_hip.so (`seva.ops`); there is no PyTorch/CPU fallback for those.
  * Host logic on O(T) / O(1000) scalars (sigma schedule, nearest-sigma lookup, per-frame CFG
    scale rule) stays in torch/numpy exactly as in the reference; the step-invariant parts are
    hoisted (the CFG scale vector is cached per (c2w, K, mask)), which also removes the per-step
    host syncs listed in SURVEY.md §7 hard part 4.
  * The per-step Gaussian draw keeps the reference's semantics (`torch.randn_like` on the
    sampler state's device, sampling.py:359) but is injectable through `EulerEDMSampler.noise_fn`
    so a CPU oracle and the GPU path can be fed identical noise.
"""

from __future__ import annotations

import contextlib
import os

import numpy as np
import torch
from tqdm import tqdm

from . import _native, _stepgraph, audit, ops
from ._native import SevaNativeError


# ------------------------------------------------------------------------------- helpers
def append_dims(x: torch.Tensor, target_dims: int) -> torch.Tensor:
    """Reference sampling.py:10-17."""
    extra = target_dims - x.ndim
    if extra < 0:
        raise ValueError(f"input has {x.ndim} dims but target_dims is {target_dims}, which is less")
    return x[(...,) + (None,) * extra]


def append_zero(x: torch.Tensor) -> torch.Tensor:
    return torch.cat([x, x.new_zeros([1])])


def to_d(x: torch.Tensor, sigma: torch.Tensor, denoised: torch.Tensor) -> torch.Tensor:
    """(x - denoised) / sigma, reference sampling.py:24-25."""
    _need_gpu(x, denoised)
    x, denoised = _f32c(x), _f32c(denoised)
    out = torch.empty_like(x)
    ops.to_d(x, denoised, _f32c(sigma), out)
    return out


def make_betas(num_timesteps: int, linear_start: float = 1e-4, linear_end: float = 2e-2) -> np.ndarray:
    return (
        torch.linspace(linear_start**0.5, linear_end**0.5, num_timesteps, dtype=torch.float64) ** 2
    ).numpy()


def generate_roughly_equally_spaced_steps(num_substeps: int, max_step: int) -> np.ndarray:
    return np.linspace(max_step - 1, 0, num_substeps, endpoint=False).astype(int)[::-1]


def _need_gpu(*tensors) -> None:
    for t in tensors:
        if isinstance(t, torch.Tensor) and not t.is_cuda:
            raise SevaNativeError(
                "seva.sampling runs its tensor math in HIP kernels: tensors must live on the GPU "
                "(no CPU fallback)."
            )


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).contiguous()


# ----------------------------------------------------------------------- discretisation
class EpsScaling(object):
    """Reference sampling.py:46-54 (vectors of length batch; host-sized math)."""

    def __call__(self, sigma: torch.Tensor):
        c_skip = torch.ones_like(sigma, device=sigma.device)
        c_out = -sigma
        c_in = 1 / (sigma**2 + 1.0) ** 0.5
        c_noise = sigma.clone()
        return c_skip, c_out, c_in, c_noise


class DDPMDiscretization(object):
    """Reference sampling.py:57-102: sqrt-linear betas -> alpha-bar -> sigma * e^{log_snr_shift}."""

    def __init__(
        self,
        linear_start: float = 5e-06,
        linear_end: float = 0.012,
        num_timesteps: int = 1000,
        log_snr_shift: float | None = 2.4,
    ):
        self.num_timesteps = num_timesteps
        self.log_snr_shift = log_snr_shift
        betas = make_betas(num_timesteps, linear_start=linear_start, linear_end=linear_end)
        self.alphas_cumprod = np.cumprod(1.0 - betas, axis=0)

    def get_sigmas(self, n: int, device: str | torch.device = "cpu") -> torch.Tensor:
        if n < self.num_timesteps:
            acp = self.alphas_cumprod[generate_roughly_equally_spaced_steps(n, self.num_timesteps)]
        elif n == self.num_timesteps:
            acp = self.alphas_cumprod
        else:
            raise ValueError(f"Expected n <= {self.num_timesteps}, but got n = {n}.")
        sigmas = ((1 - acp) / acp) ** 0.5
        if self.log_snr_shift is not None:
            sigmas = sigmas * np.exp(self.log_snr_shift)
        return torch.flip(torch.tensor(sigmas, dtype=torch.float32, device=device), (0,))

    def __call__(self, n: int, do_append_zero: bool = True, flip: bool = False,
                 device: str | torch.device = "cpu") -> torch.Tensor:
        sigmas = self.get_sigmas(n, device=device)
        sigmas = append_zero(sigmas) if do_append_zero else sigmas
        return sigmas if not flip else torch.flip(sigmas, (0,))


class DiscreteDenoiser(object):
    """Reference sampling.py:105-152."""

    sigmas: torch.Tensor

    def __init__(self, discretization: DDPMDiscretization, num_idx: int = 1000,
                 device: str | torch.device = "cpu"):
        self.scaling = EpsScaling()
        self.discretization = discretization
        self.num_idx = num_idx
        self.device = device
        self.register_sigmas()

    def register_sigmas(self):
        self.sigmas = self.discretization(self.num_idx, do_append_zero=False, flip=True, device=self.device)

    def sigma_to_idx(self, sigma: torch.Tensor) -> torch.Tensor:
        dists = sigma - self.sigmas[:, None]
        return dists.abs().argmin(dim=0).view(sigma.shape)

    def idx_to_sigma(self, idx: torch.Tensor | int) -> torch.Tensor:
        return self.sigmas[idx]

    def __call__(self, network, input: torch.Tensor, sigma: torch.Tensor, cond: dict,
                 **additional_model_inputs) -> torch.Tensor:
        _need_gpu(input, sigma)
        sigma = self.idx_to_sigma(self.sigma_to_idx(sigma))  # (B,) nearest table entries
        c_skip, c_out, c_in, c_noise = self.scaling(sigma)
        c_noise = self.sigma_to_idx(c_noise)
        x = _f32c(input)
        if "replace" in cond:
            rep = _f32c(cond.pop("replace"))
            assert rep.shape[1] == x.shape[1] + 1
            blended = torch.empty_like(x)
            ops.replace_blend(x, rep, blended)  # x*(1-mask) + latent*mask
            x = blended
        x_in = torch.empty_like(x)
        ops.scale_rows(x, _f32c(c_in), x_in)
        net = network(x_in, c_noise, cond, **additional_model_inputs)
        out = torch.empty_like(x)
        ops.denoiser_combine(_f32c(net), x, _f32c(c_out), _f32c(c_skip), out)
        return out


# ------------------------------------------------------------------------------ guiders
def get_camera_dist(source_c2ws: torch.Tensor, target_c2ws: torch.Tensor, mode: str = "translation"):
    """Pairwise camera distance (reference seva/geometry.py:12-40); O(N*M) host-sized math."""
    if mode == "rotation":
        rel = torch.matmul(source_c2ws[:, None, :3, :3], target_c2ws[None, :, :3, :3].transpose(-1, -2))
        cos = (rel.diagonal(offset=0, dim1=-2, dim2=-1).sum(-1) - 1) / 2
        return torch.acos(cos.clamp(-1, 1)) * (180 / torch.pi)
    if mode == "translation":
        return torch.norm(source_c2ws[:, None, :3, 3] - target_c2ws[None, :, :3, 3], dim=-1)
    raise NotImplementedError(f"Mode {mode} is not implemented for finding nearest source indices.")


class ConstantScaleRule(object):
    def __call__(self, scale):
        return scale


class MultiviewScaleRule(object):
    """Reference sampling.py:160-187: frames that coincide with an input view get `min_scale`."""

    def __init__(self, min_scale: float = 1.0):
        self.min_scale = min_scale

    def __call__(self, scale, c2w: torch.Tensor, K: torch.Tensor, input_frame_mask: torch.Tensor):
        c2w_input = c2w[input_frame_mask]
        rotation_diff = get_camera_dist(c2w, c2w_input, mode="rotation").min(-1).values
        translation_diff = get_camera_dist(c2w, c2w_input, mode="translation").min(-1).values
        K_diff = ((K[:, None] - K[input_frame_mask][None]).flatten(-2) == 0).all(-1).any(-1)
        close_frame = (rotation_diff < 10.0) & (translation_diff < 1e-5) & K_diff
        if isinstance(scale, torch.Tensor):
            scale = scale.clone()
            scale[close_frame] = self.min_scale
        elif isinstance(scale, float):
            scale = torch.where(close_frame, self.min_scale, scale)
        else:
            raise ValueError(f"Invalid scale type {type(scale)}.")
        return scale


class ConstantScaleSchedule(object):
    def __call__(self, sigma, scale):
        if isinstance(sigma, float):
            return scale
        elif isinstance(sigma, torch.Tensor):
            if len(sigma.shape) == 1 and isinstance(scale, torch.Tensor):
                sigma = append_dims(sigma, scale.ndim)
            return scale * torch.ones_like(sigma)
        else:
            raise ValueError(f"Invalid sigma type {type(sigma)}.")


class ConstantGuidance(object):
    """uncond + scale*(cond - uncond), reference sampling.py:204-213 -- one HIP kernel."""

    def __call__(self, uncond: torch.Tensor, cond: torch.Tensor, scale) -> torch.Tensor:
        den2 = torch.cat([uncond, cond], 0)
        return _cfg_combine(den2, scale)


def _scale_vector(scale, n: int, device) -> torch.Tensor:
    """Any reference-style scale value (float, (n,), (n,1,1,1)) -> contiguous f32 (n,)."""
    if isinstance(scale, torch.Tensor):
        s = scale.to(device=device, dtype=torch.float32).reshape(-1)
        if s.numel() == 1:
            s = s.expand(n)
        if s.numel() != n:
            raise ValueError(f"guidance scale has {s.numel()} entries for {n} frames")
        return s.contiguous()
    return torch.full((n,), float(scale), device=device, dtype=torch.float32)


def _cfg_combine(den2: torch.Tensor, scale) -> torch.Tensor:
    _need_gpu(den2)
    den2 = _f32c(den2)
    n = den2.shape[0] // 2
    out = torch.empty((n,) + tuple(den2.shape[1:]), device=den2.device, dtype=torch.float32)
    ops.cfg_combine(den2, _scale_vector(scale, n, den2.device), out)
    return out


class VanillaCFG(object):
    """Reference sampling.py:216-242."""

    def __init__(self):
        self.scale_rule = ConstantScaleRule()
        self.scale_schedule = ConstantScaleSchedule()
        self.guidance = ConstantGuidance()

    # the per-frame guidance weight; everything below it is step-invariant
    def frame_scale(self, x: torch.Tensor, sigma, scale, **_):
        return self.scale_schedule(sigma, self.scale_rule(scale))

    def __call__(self, x: torch.Tensor, sigma, scale) -> torch.Tensor:
        return _cfg_combine(x, self.frame_scale(x, sigma, scale))

    def prepare_inputs(self, x: torch.Tensor, s: torch.Tensor, c: dict, uc: dict):
        c_out = dict()
        for k in c:
            if k in ["vector", "crossattn", "concat", "replace", "dense_vector"]:
                c_out[k] = torch.cat((uc[k], c[k]), 0)
            else:
                assert c[k] == uc[k]
                c_out[k] = c[k]
        return torch.cat([x] * 2), torch.cat([s] * 2), c_out


class MultiviewCFG(VanillaCFG):
    """Reference sampling.py:245-265."""

    def __init__(self, cfg_min: float = 1.0):
        self.scale_min = cfg_min
        self.scale_rule = MultiviewScaleRule(min_scale=cfg_min)
        self.scale_schedule = ConstantScaleSchedule()
        self.guidance = ConstantGuidance()
        self._rule_cache: tuple | None = None

    def reset_rule_cache(self) -> None:
        """Called by `EulerEDMSampler.prepare_sampling_loop`: a new trajectory never reuses an old rule."""
        self._rule_cache = None

    def _rule(self, scale, c2w, K, input_frame_mask, ndim):
        """The step-invariant per-frame scale (the hook subclasses override; this rule has no use for `ndim`)."""
        return self.scale_rule(scale, c2w, K, input_frame_mask)

    def _ruled_scale(self, scale, c2w, K, input_frame_mask, ndim):
        """`_rule(...)`, whose boolean-mask indexing is a host sync that must not sit inside a captured step, evaluated once
        per trajectory.

        The cache entry keeps STRONG references to the very tensor objects it was computed from and matches by
        object identity (`is`), so an address the caching allocator hands out again for another scene can never
        alias an entry, and nothing here reads `_version` (inference tensors -- reference eval.py:1242 creates
        c2w / K / mask under torch.inference_mode() -- do not track one).  `do_sample` passes the same tensor
        objects on every step of a trajectory (eval.py:1285-1312), which is what makes the hit path the common one;
        in-place edits of those tensors between steps are not part of the reference's contract."""
        ent = self._rule_cache
        if ent is not None:
            (s0, a0, b0, m0), val = ent
            same_scale = (s0 is scale) if isinstance(scale, torch.Tensor) else (
                not isinstance(s0, torch.Tensor) and s0 == scale)
            if same_scale and a0 is c2w and b0 is K and m0 is input_frame_mask:
                return val
        val = self._rule(scale, c2w, K, input_frame_mask, ndim)
        self._rule_cache = ((scale, c2w, K, input_frame_mask), val)
        return val

    def frame_scale(self, x, sigma, scale, c2w=None, K=None, input_frame_mask=None, **_):
        return self.scale_schedule(sigma, self._ruled_scale(scale, c2w, K, input_frame_mask, x.ndim))

    def __call__(self, x: torch.Tensor, sigma, scale, c2w: torch.Tensor, K: torch.Tensor,  # type: ignore
                 input_frame_mask: torch.Tensor) -> torch.Tensor:
        return _cfg_combine(x, self.frame_scale(x, sigma, scale, c2w, K, input_frame_mask))


class MultiviewTemporalCFG(MultiviewCFG):
    """Reference sampling.py:268-298: scale additionally ramps with index distance to an input."""

    def __init__(self, num_frames: int, cfg_min: float = 1.0):
        super().__init__(cfg_min=cfg_min)
        self.num_frames = num_frames
        idx = torch.arange(num_frames)
        self.distance_matrix = (idx[None] - idx[:, None]).abs()

    def _rule(self, scale, c2w, K, input_frame_mask, ndim):
        """Temporal ramp, then the close-frame rule: step-invariant like the base's, and cached by it in the same way."""
        mask = input_frame_mask.reshape(-1, self.num_frames)
        min_distance = (
            self.distance_matrix[None].to(mask.device) + (~mask[:, None]) * self.num_frames
        ).min(-1)[0]
        min_distance = min_distance / min_distance.max(-1, keepdim=True)[0].clamp(min=1)
        ramp = min_distance * (scale - self.scale_min) + self.scale_min
        ramp = append_dims(ramp.reshape(-1), ndim)
        return self.scale_rule(ramp, c2w, K, mask.flatten(0, 1))


# ------------------------------------------------------------------------------ sampler
SOLVERS = ("euler", "dpmpp2m")


def parse_cache(interval, levels) -> tuple:
    """(interval, levels) of the deep-feature reuse from arguments or environment strings: interval None / "" / 0 / 1 = off
    (returned as 0), N >= 2 = on; levels 1, 2 or 3 (None / "": 1).  Anything else is a ValueError."""
    def as_int(v, what):
        if isinstance(v, bool) or not isinstance(v, (int, str)):
            raise ValueError(f"{what} must be an integer, got {v!r}")
        try:
            return int(v)
        except ValueError:
            raise ValueError(f"{what} must be an integer, got {v!r}") from None

    n = 0 if interval is None or interval == "" else as_int(interval, "cache_interval")
    lv = 1 if levels is None or levels == "" else as_int(levels, "cache_levels")
    if n < 0:
        raise ValueError(f"cache_interval must be 0 or 1 (off) or >= 2, got {interval!r}")
    if lv not in (1, 2, 3):
        raise ValueError(f"cache_levels must be 1, 2 or 3, got {levels!r}")
    return (n if n >= 2 else 0), lv


def parse_guidance(interval, rescale) -> tuple:
    """(interval, phi) of the guidance controls from arguments or environment strings.  interval: None / "" = off (returned as
    None), else (sigma_lo, sigma_hi) -- a pair of numbers or a string "lo,hi" -- with 0 <= sigma_lo < sigma_hi, sigma_hi may be
    inf; returned as a pair of floats.  rescale: None / "" = 0.0 (off), else a number or numeric string in [0, 1].  Anything else
    is a ValueError."""
    def as_float(v, what):
        if isinstance(v, bool) or not isinstance(v, (int, float, str)):
            raise ValueError(f"{what} must be a number, got {v!r}")
        try:
            f = float(v)
        except ValueError:
            raise ValueError(f"{what} must be a number, got {v!r}") from None
        if f != f:
            raise ValueError(f"{what} must not be NaN")
        return f

    if interval is None or (isinstance(interval, str) and interval.strip() == ""):
        iv = None
    else:
        parts = interval.split(",") if isinstance(interval, str) else interval
        if not isinstance(parts, (list, tuple)) or len(parts) != 2:
            raise ValueError(f"guidance_interval must be (sigma_lo, sigma_hi) or \"lo,hi\", got {interval!r}")
        lo, hi = as_float(parts[0], "guidance_interval sigma_lo"), as_float(parts[1], "guidance_interval sigma_hi")
        if not (0.0 <= lo < hi) or lo == float("inf"):
            raise ValueError(f"guidance_interval needs 0 <= sigma_lo < sigma_hi, got {interval!r}")
        iv = (lo, hi)
    if rescale is None or (isinstance(rescale, str) and rescale.strip() == ""):
        phi = 0.0
    else:
        phi = as_float(rescale, "guidance_rescale")
        if not 0.0 <= phi <= 1.0:
            raise ValueError(f"guidance_rescale must lie in [0, 1], got {rescale!r}")
    return iv, phi


def resolve_options(solver=None, cache_interval=None, cache_levels=1, guidance_interval=None, guidance_rescale=None) -> dict:
    """The opt-in options of `EulerEDMSampler` (its docstring says what each does), from arguments and environment, as the attributes
    the sampler holds.  The only place that names the SEVA_* variables of the sampler: an argument that is None reads its variable,
    any other argument wins over it.  SEVA_CACHE_LEVELS is read together with SEVA_CACHE_INTERVAL, that is only where
    `cache_interval` is None, and where it is unset or empty the depth is the argument; an empty SEVA_SOLVER is unset too."""
    env = os.environ.get
    if guidance_interval is None:
        guidance_interval = env("SEVA_GUIDANCE_INTERVAL")
    if guidance_rescale is None:
        guidance_rescale = env("SEVA_GUIDANCE_RESCALE")
    guidance_interval, guidance_rescale = parse_guidance(guidance_interval, guidance_rescale)
    if cache_interval is None:
        cache_interval, cache_levels = env("SEVA_CACHE_INTERVAL"), env("SEVA_CACHE_LEVELS") or cache_levels
    cache_interval, cache_levels = parse_cache(cache_interval, cache_levels)
    if solver is None:
        solver = env("SEVA_SOLVER") or "euler"
    if solver not in SOLVERS:
        raise ValueError(f"unknown solver {solver!r}: expected one of {SOLVERS}")
    return dict(solver=solver, cache_interval=cache_interval, cache_levels=cache_levels, guidance_interval=guidance_interval,
                guidance_rescale=guidance_rescale)


def per_pass(v) -> tuple:
    """One value or a (first pass, second pass) pair -> the pair (the reference's `--T N,21`, `cfg 3,2`; eval.py:1785-1789)."""
    if isinstance(v, (list, tuple)):
        assert len(v) == 2, f"one value or a (first pass, second pass) pair, not {v!r}"
        return v[0], v[1]
    return v, v


def per_pass_options(solver=None, cache_interval=None, cache_levels=1, guidance_interval=None, guidance_rescale=None) -> tuple:
    """The two-pass drivers' sampler options -> (first pass, second pass): the `EulerEDMSampler` keywords of each pass's windows.
    Every option but `solver` takes one value or a pair (`per_pass`).  One value of `guidance_interval` is itself a 2-tuple
    (`parse_guidance`), so there a pair is a 2-tuple whose elements are each None, a (lo, hi) tuple or a "lo,hi" string; anything
    else -- None, a string, a 2-tuple of numbers -- is one interval for both passes.  `solver` is one value for the trajectory."""
    iv = guidance_interval
    if not (isinstance(iv, (list, tuple)) and len(iv) == 2 and all(e is None or isinstance(e, (list, tuple, str)) for e in iv)):
        iv = (iv, iv)
    pairs = dict(cache_interval=per_pass(cache_interval), cache_levels=per_pass(cache_levels), guidance_interval=iv,
                 guidance_rescale=per_pass(guidance_rescale))
    return tuple({"solver": solver, **{k: v[p] for k, v in pairs.items()}} for p in (0, 1))


def step_kinds(sigmas_host, cache_interval: int, cache_levels: int, guidance_interval: tuple | None) -> list:
    """The step schedule of a trajectory: per step, the keywords `EulerEDMSampler.__call__` adds to `sampler_step` -- {} for a full
    guided step, {"shallow": L} for a shallow one, {"guided": False} for an unguided one, both where both hold.  `sigmas_host`: the
    schedule's sigmas with the final 0, on the host; the other arguments as `resolve_options` returns them.
    Deep-feature reuse: a full step at every `cache_interval`-th step and at the last one, shallow steps in between; and a shallow
    call needs a full call of the same batch behind it, so a step whose guided flag differs from the previous step's is full too.
    Guidance interval: decided on the schedule's own sigma (not sigma_hat: churn moves no step across a bound), in the sigmas' dtype
    like the s_tmin / s_tmax test (`prepare_sampling_loop`).
    A keyword is absent while its feature is off: the calls are then the ones made before, and a subclass's `sampler_step` never
    sees the keyword."""
    kinds, last, was_guided = [], len(sigmas_host) - 2, True
    for i in range(len(sigmas_host) - 1):
        guided = guidance_interval is None or bool(guidance_interval[0] < sigmas_host[i] <= guidance_interval[1])
        full = not cache_interval or i % cache_interval == 0 or i == last or guided != was_guided
        kind = {} if full else {"shallow": cache_levels}
        if not guided:
            kind["guided"] = False
        kinds.append(kind)
        was_guided = guided
    return kinds


def _network_depth(levels: int):
    """Context of one network call at depth `levels`: L > 0 is `_native.shallow_network(L)`, 0 (the whole network) changes nothing."""
    return _native.shallow_network(levels) if levels else contextlib.nullcontext()


class EulerEDMSampler(object):
    """Reference sampling.py:301-405 (Euler discretisation of the EDM probability-flow ODE).

    `solver` (opt-in, not in the reference): "euler" = the reference's step; "dpmpp2m" = DPM-Solver++(2M), the
    deterministic second-order multistep solver (`DPMPP2MSampler` of sgm), same one network call per step.  None reads
    the environment variable SEVA_SOLVER (default "euler"), so code that constructs or subclasses this class by name can
    opt in unchanged; an explicit argument wins over the variable.

    `cache_interval` = N >= 2 (opt-in, not in the reference): reuse of deep UNet features across steps.  Step i of a trajectory
    runs the whole network iff i % N == 0 or it is the last step; every other step runs a shallow network call of depth
    `cache_levels` (1, 2 or 3: `SevaEngine.forward(shallow_levels=...)`), which recomputes the top of the UNet and takes the rest
    from the last full step.  0 or 1: off.  None reads SEVA_CACHE_INTERVAL and SEVA_CACHE_LEVELS (unset: off, depth 1).  The
    schedule (`step_kinds`) is followed by `__call__`: a subclass that drives `sampler_step` itself gets full steps.

    `guidance_interval` = (sigma_lo, sigma_hi) (opt-in, not in the reference; Kynkaanniemi et al. 2024): step i is guided iff
    sigma_lo < sigmas[i] <= sigma_hi -- the schedule's own sigma, so churn moves no step across a bound.  Every other step calls the
    denoiser on the conditional inputs alone (n frames instead of 2n, no guider) and takes the plain update.  None reads
    SEVA_GUIDANCE_INTERVAL="lo,hi" (unset: off = every step guided).  This is part of `step_kinds` too: a subclass that drives
    `sampler_step` itself gets guided steps.  With `cache_interval`, a step whose guided flag differs from the previous step's is a
    full step as well (the network's batch changes there).
    `guidance_rescale` = phi in [0, 1] (opt-in, not in the reference; Lin et al. 2024): on guided steps the guided prediction of
    each frame is scaled to the standard deviation of that frame's conditional prediction, blended with weight phi
    (`ops.cfg_rescale`), before the plain update.  None reads SEVA_GUIDANCE_RESCALE (unset or 0: off).  Needs a guider that states
    its `frame_scale`."""

    def __init__(self, discretization: DDPMDiscretization, guider, num_steps: int | None = None,
                 verbose: bool = False, device: str | torch.device = "cuda", s_churn=0.0, s_tmin=0.0,
                 s_tmax=float("inf"), s_noise=1.0, solver: str | None = None, check_finite: bool | None = None,
                 cache_interval: int | None = None, cache_levels: int | None = 1,
                 guidance_interval: tuple | str | None = None, guidance_rescale: float | None = None):
        # plain attributes (assignable afterwards): solver, cache_interval, cache_levels, guidance_interval, guidance_rescale
        vars(self).update(resolve_options(solver, cache_interval, cache_levels, guidance_interval, guidance_rescale))
        if self.solver == "dpmpp2m" and s_churn > 0:
            raise ValueError("solver 'dpmpp2m' is deterministic: it has no stochastic form here, s_churn must be 0")
        # True: one ops.tensor_range over the final latent after the last step; an inf / NaN raises.  None: SEVA_CHECK_FINITE=1.  Off by default
        self.check_finite = audit.check_finite_from_env() if check_finite is None else bool(check_finite)
        # multistep history (dpmpp2m only): the previous step's guided denoised latent D-, its sigma, and whether they are valid.
        # Owned by the sampler and cleared by `prepare_sampling_loop`; the buffer itself persists (the whole-step hipGraph holds
        # its address) and is never read while `_ms_have` is False.
        self._ms_den: torch.Tensor | None = None
        self._ms_sigma: torch.Tensor | None = None
        self._ms_have = False
        self.num_steps = num_steps
        self.discretization = discretization
        self.guider = guider
        self.verbose = verbose
        self.device = device
        self.s_churn = s_churn
        self.s_tmin = s_tmin
        self.s_tmax = s_tmax
        self.s_noise = s_noise
        self.noise_fn = torch.randn_like  # injectable: fn(x) -> N(0,1) tensor like x
        self._step_graphs = _stepgraph.StepGraphCache()
        # CFG-split (strong scaling of ONE window over two GPUs): (process group of two ranks, half) with
        # half = this rank's position in the group: 0 runs the unconditional half of the CFG batch, 1 the conditional half.
        # Each step the two ranks all-gather their (T,4,h,w) denoised halves (435 KB at 576x576 over xGMI) and then both
        # perform the identical guidance + Euler update, so both hold the full sampler state; the per-step noise must come
        # from identically seeded generators on both ranks (`noise_fn`; seva.pipeline does that).  None = the whole CFG batch
        # on this rank (the reference's single-process semantics, sampling.py:231-242).
        self.cfg_split: tuple | None = None

    def prepare_sampling_loop(self, x: torch.Tensor, cond: dict, uc: dict, num_steps: int | None = None):
        num_steps = num_steps or self.num_steps
        assert num_steps is not None, "num_steps must be specified"
        _need_gpu(x)
        if hasattr(self.guider, "reset_rule_cache"):
            self.guider.reset_rule_cache()
        self._ms_sigma, self._ms_have = None, False  # a new trajectory starts without multistep history
        sigmas = self.discretization(num_steps, device=self.device)
        # x *= sqrt(1 + sigma_0^2), in place on the caller's tensor like the reference (l.331)
        s0 = torch.sqrt(1.0 + sigmas[0] ** 2.0).to(device=x.device, dtype=torch.float32)
        s0 = s0.expand(x.shape[0]).contiguous()
        if x.dtype == torch.float32 and x.is_contiguous():
            ops.scale_rows(x, s0, x)
        else:
            tmp = _f32c(x)
            ops.scale_rows(tmp, s0, tmp)
            x.copy_(tmp)
        num_sigmas = len(sigmas)
        s_in = x.new_ones([x.shape[0]])
        # host copy so the per-step s_tmin/s_tmax test never syncs with the device.  It keeps the sigmas' dtype: the reference
        # compares a tensor element with the bounds (l.391), so a bound is rounded to fp32 before the comparison, and a Python
        # double would put a step on the other side of a bound that lies within half an fp32 ulp of its sigma
        self._sigmas_host = sigmas.detach().cpu()
        return x, s_in, sigmas, num_sigmas, cond, uc

    def get_sigma_gen(self, num_sigmas: int, verbose: bool = True):
        sigma_generator = range(num_sigmas - 1)
        if self.verbose and verbose:
            sigma_generator = tqdm(sigma_generator, total=num_sigmas - 1, desc="Sampling", leave=False)
        return sigma_generator

    def _step_math(self, sigma, next_sigma, x, eps, gamma, operands):
        """Reference sampling.py:357-368 on f32 contiguous device tensors; sync-free once the guider's rule is cached,
        which is what makes it capturable as one hipGraph (`_stepgraph.StepGraph`).  The step's kind (shallow, guided,
        `guidance_rescale`) decides the operands alone: `operands(x_in, sigma_in)` is `sampler_step`'s `_step_operands`."""
        sigma_hat = sigma * (gamma + 1.0) + 1e-6
        noise_scale = (sigma_hat**2 - sigma**2) ** 0.5 * self.s_noise
        x_noised = torch.empty_like(x)
        ops.add_noise(x, eps, _f32c(noise_scale), x_noised)
        den, fs = operands(x_noised, sigma_hat)
        dt = next_sigma - sigma_hat
        out = torch.empty_like(x)
        if fs is not None:
            ops.cfg_euler(x_noised, den, fs, sigma_hat, dt, out)  # CFG combine + to_d + Euler update in one pass
        else:
            ops.euler_step(x_noised, den, sigma_hat, dt, out)
        return out

    def _denoised_pair(self, denoiser, x_in, sigma_in, cond, uc):
        """The [uncond ; cond] denoised latents for (x_in, sigma_in): one CFG-batched network call, or under `cfg_split`
        this rank's half of it and the other rank's."""
        if self.cfg_split is None:
            return denoiser(*self.guider.prepare_inputs(x_in, sigma_in, cond, uc))
        return self._denoise_cfg_split(denoiser, x_in, sigma_in, cond, uc)

    def _step_operands(self, denoiser, x_in, sigma_in, scale, cond, uc, guider_kwargs, shallow=0, guided=True):
        """(den, fs) for a step's update kernel, whatever the step's kind.  `shallow` = L > 0: the step's one network call, guided
        or not, runs at depth L (`_network_depth`; under `cfg_split` on either rank: each owns an engine, both follow one schedule).
        Guided, `guidance_rescale` 0: `_guidance_operands` of the CFG-batched call -- the fused kernels combine.
        Guided, `guidance_rescale` = phi > 0: (D, None) with D from `ops.cfg_rescale` on the [uncond ; cond] pair, a latent-sized
        round trip that the fused path does not make; needs a guider that states its `frame_scale`.
        Unguided: (the denoiser on the conditional inputs alone, None), at batch n -- no `guider.prepare_inputs`, no scale rule,
        and under `cfg_split` no collective: both ranks of the pair make this call themselves and go on holding identical state
        (the half batch is bitwise the half of the full batch).  The denoiser gets a dictionary of its own (`DiscreteDenoiser`
        pops "replace" from the one it is handed)."""
        phi = self.guidance_rescale
        if guided and phi > 0 and not hasattr(self.guider, "frame_scale"):
            raise ValueError("guidance_rescale > 0 needs a guider that states its per-frame scale (`frame_scale`): "
                             f"{type(self.guider).__name__} has none")
        with _network_depth(shallow):
            if not guided:
                return _f32c(denoiser(x_in, sigma_in, dict(cond))), None
            denoised2 = self._denoised_pair(denoiser, x_in, sigma_in, cond, uc)
        den, fs = self._guidance_operands(denoised2, sigma_in, scale, x_in, guider_kwargs)
        if phi > 0:
            D = torch.empty_like(x_in)
            ops.cfg_rescale(den, fs, phi, D)
            return D, None
        return den, fs

    def _guidance_operands(self, denoised2, sigma_in, scale, x, guider_kwargs):
        """What the fused update kernels take: (the f32 [uncond ; cond] pair, the per-frame scale vector) for them to
        combine themselves where the guider can state its `frame_scale`, (the guider's own guided latent, None) where
        it cannot."""
        if hasattr(self.guider, "frame_scale"):
            fs = self.guider.frame_scale(denoised2, sigma_in, scale, **guider_kwargs)
            return _f32c(denoised2), _scale_vector(fs, x.shape[0], x.device)
        return _f32c(self.guider(denoised2, sigma_in, scale, **guider_kwargs)), None

    def _denoise_cfg_split(self, denoiser, x_noised, sigma_hat, cond, uc):
        """[uncond ; cond] denoised latents with each half of the CFG batch computed by one rank of `cfg_split`'s
        two-rank group and exchanged by ONE all-gather (rank order of the group = batch order of
        `VanillaCFG.prepare_inputs`, reference sampling.py:231-242).  Every row of the network's output depends only on
        the rows of its own scene, and the kernels' tilings are chosen from per-sample sizes, so the half batch is bitwise
        the corresponding half of the full batch."""
        import torch.distributed as dist

        group, half = self.cfg_split
        xx, ss, cc = self.guider.prepare_inputs(x_noised, sigma_hat, cond, uc)
        n = x_noised.shape[0]
        sl = slice(half * n, (half + 1) * n)
        cc_half = {k: (v[sl] if isinstance(v, torch.Tensor) and v.dim() > 0 and v.shape[0] == 2 * n else v) for k, v in cc.items()}
        mine = _f32c(denoiser(xx[sl], ss[sl], cc_half))
        both = torch.empty((2 * n,) + tuple(mine.shape[1:]), dtype=mine.dtype, device=mine.device)
        if mine.is_cuda and dist.get_backend(group) == "gloo":
            # rehearsal backend only (RCCL is stream-ordered): gloo stages device tensors through the host, and with the half-batch
            # network still in flight its all-gather took 5.5 s per step on a shared card instead of 3 ms (profiles/r03_bench_n2_rehearsal*)
            torch.cuda.synchronize(mine.device)
        dist.all_gather_into_tensor(both, mine, group=group)
        return both

    @staticmethod
    def multistep_coefficients(sigma: torch.Tensor, next_sigma: torch.Tensor, prev_sigma: torch.Tensor):
        """DPM-Solver++(2M) coefficients as f32 vectors on the sigmas' device, without a host sync:
        x+ = a x + b D + c D-.   a = s+/s.   Rows without history (prev_sigma <= 0) and rows that land on s+ = 0:
        b = 1 - a, c = 0 (the first-order / DDIM step; with s+ = 0 exactly a = 0, b = 1).   Otherwise, with
        r = ln(s-/s) / ln(s/s+):  b = (1 - a)(1 + 1/(2r)),  c = -(1 - a)/(2r)   (sgm: mult1 = a, mult2 = -(1 - a),
        mult3 = 1 + 1/(2r), mult4 = 1/(2r))."""
        a = next_sigma / sigma
        one_a = 1.0 - a
        second = (prev_sigma > 0) & (next_sigma > 0)
        # rows where `second` is False evaluate logs of 0 or of a negative ratio; torch.where discards them
        inv_2r = torch.log(sigma / next_sigma) / (2.0 * torch.log(prev_sigma / sigma))
        zero = torch.zeros_like(a)
        b = torch.where(second, one_a * (1.0 + inv_2r), one_a)
        c = torch.where(second, -one_a * inv_2r, zero)
        return a, b, c

    def _multistep_math(self, sigma, next_sigma, x, prev_sigma, hist, operands):
        """One DPM-Solver++(2M) step on f32 contiguous device tensors: no noise, no sigma_hat; guidance, update and the new
        history in ONE kernel (`ops.cfg_multistep`), which reads D- from `hist` and leaves D there.  Sync-free like
        `_step_math`, and the same code for the first, the second-order and the last step (they differ in a, b, c only), so
        one hipGraph serves them all.  An unguided or a rescaled step hands the kernel its D with scale=None
        (`_step_operands`); the history is whatever D the step used."""
        den, fs = operands(x, sigma)
        a, b, c = self.multistep_coefficients(sigma, next_sigma, prev_sigma)
        out = torch.empty_like(x)
        ops.cfg_multistep(x, den, fs, hist, a, b, c, out, hist)
        return out

    def _multistep_history(self, x, sigma):
        """(the history buffer D-, the previous step's sigma or 0 = "no history" to the coefficients) for one dpmpp2m step."""
        hist = self._ms_den
        if hist is None or hist.shape != x.shape or hist.device != x.device:
            # an ordinary tensor even under torch.inference_mode(), like the static buffers of `_stepgraph.StepGraph`
            with torch.inference_mode(False):
                hist = self._ms_den = torch.zeros(x.shape, dtype=torch.float32, device=x.device)
            self._ms_have = False
        return hist, (self._ms_sigma if self._ms_have else torch.zeros_like(sigma))

    def _whole_step_graph_eligible(self, x) -> bool:
        """Whether this step goes through the whole-step hipGraph protocol (`_stepgraph.StepGraphCache.run`)."""
        # (CFG-split steps are not captured as one graph: the per-step all-gather runs eagerly between the two ranks;
        #  the network call itself is still replayed from its own hipGraph)
        # (under an audit recorder the step is neither captured nor replayed: its launches must run, and be seen, one by one)
        return (x.is_cuda and not self._step_graphs.disabled and _stepgraph.enabled() and self.cfg_split is None
                and ops._AUDIT is None and not torch.cuda.is_current_stream_capturing())

    def sampler_step(self, sigma: torch.Tensor, next_sigma: torch.Tensor, denoiser, x: torch.Tensor,
                     scale, cond: dict, uc: dict, gamma: float = 0.0, *, shallow: int = 0, guided: bool = True,
                     **guider_kwargs) -> torch.Tensor:
        """One Euler-EDM step (reference sampling.py:347-368), or one DPM-Solver++(2M) step under solver="dpmpp2m".  From
        the second step of a trajectory on, the whole step is replayed from one hipGraph (see `_stepgraph`); the first step
        runs eagerly and warms every cache.  Stays a callable unit for `GradioTrackedSampler` (reference eval.py:1037-1089).
        `shallow` = L > 0 (`__call__`'s `cache_interval` schedule): the step's network call is a shallow one of depth L; such
        steps have a whole-step graph of their own.  `guided` False (`__call__`'s `guidance_interval` schedule): the step calls the
        denoiser on the conditional inputs alone and takes the plain update; such steps, full or shallow, have graphs of their
        own too."""
        _need_gpu(x)
        x = _f32c(x)
        sigma = _f32c(sigma)
        next_sigma = _f32c(next_sigma)
        multistep = self.solver == "dpmpp2m"
        flat = _stepgraph.StepGraphCache.flat_key((scale, cond, uc, guider_kwargs))
        # what the feature adds to the key, nothing while it is off: a rescaled step's phi is baked into its graph
        if not guided:
            flat += ("unguided",)
        elif self.guidance_rescale > 0:
            flat += ("rescale", float(self.guidance_rescale))
        operands = lambda x_in, sigma_in: self._step_operands(denoiser, x_in, sigma_in, scale, cond, uc, guider_kwargs, shallow, guided)  # noqa: E731
        # per solver: the cache key (everything the closure holds), the sync-free step as a closure, the fourth graph input
        if multistep:  # deterministic: no noise draw, no add_noise; `gamma` has nothing to act on
            hist, fourth = self._multistep_history(x, sigma)
            key = ("dpmpp2m", tuple(x.shape), hist, self.guider, denoiser) + flat
            fn = lambda s, n, xx, ps: self._multistep_math(s, n, xx, ps, hist, operands)  # noqa: E731
        else:
            fourth = _f32c(self.noise_fn(x))  # eps, drawn eagerly: the generator advances per step exactly as in the reference
            gamma = float(gamma)
            key = (tuple(x.shape), gamma, float(self.s_noise), self.guider, denoiser) + flat
            fn = lambda s, n, xx, ee: self._step_math(s, n, xx, ee, gamma, operands)  # noqa: E731
        # the step kind names the graph entry: 0 / L as ever for a guided step, (0 / L, "unguided") for an unguided one
        kind = shallow if guided else (shallow, "unguided")
        # keep: the graph reads the warm-up step's rule tensor, which must therefore outlive `reset_rule_cache`
        out = self._step_graphs.run(key, fn, (sigma, next_sigma, x, fourth), eligible=self._whole_step_graph_eligible(x),
                                    keep=lambda: getattr(self.guider, "_rule_cache", None), **({"kind": kind} if kind else {}))
        if multistep:
            self._ms_sigma, self._ms_have = sigma, True
        return out

    def __call__(self, denoiser, x: torch.Tensor, scale, cond: dict, uc: dict | None = None,
                 num_steps: int | None = None, verbose: bool = True, **guider_kwargs) -> torch.Tensor:
        uc = cond if uc is None else uc
        x, s_in, sigmas, num_sigmas, cond, uc = self.prepare_sampling_loop(x, cond, uc, num_steps)
        kinds = step_kinds(self._sigmas_host, self.cache_interval, self.cache_levels, self.guidance_interval)
        for i in self.get_sigma_gen(num_sigmas, verbose=verbose):
            gamma = (
                min(self.s_churn / (num_sigmas - 1), 2**0.5 - 1)
                if self.s_tmin <= self._sigmas_host[i] <= self.s_tmax
                else 0.0
            )
            x = self.sampler_step(s_in * sigmas[i], s_in * sigmas[i + 1], denoiser, x, scale, cond, uc,
                                  gamma, **kinds[i], **guider_kwargs)
        # once per trajectory, after the last step (never inside the loop): a split-K consumer that gave up waiting for its
        # producer (csrc/gemm.hip) left a wrong tile behind -- make that an error instead of a silently wrong sample
        if x.is_cuda:
            ops.check_handoffs()
            if self.check_finite:
                audit.check_finite(x)
        return x


class DPMPP2MSampler(EulerEDMSampler):
    """`EulerEDMSampler` with solver="dpmpp2m" fixed (sgm's DPMPP2MSampler; not part of the reference's sampler file)."""

    def __init__(self, *args, **kwargs):
        kwargs["solver"] = "dpmpp2m"
        super().__init__(*args, **kwargs)
