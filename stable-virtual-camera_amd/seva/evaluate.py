"""`python -m seva.evaluate`: run scene folders through a list of modes and score every mode against the held-out pictures and
against the baseline's frames.

    python -m seva.evaluate --scenes DIR[,DIR...] --task img2img --num-inputs 3 --size 576 --model DIR \\
        [--vae FILE --clip FILE --lpips-vgg FILE --lpips-lin FILE] --modes f16,fp8,cache@2 --out DIR

A mode is `+`-joined tokens of `TOKENS` below: engine settings (`Seva.set_precision`, `AutoEncoder.set_precision` /
`set_upsample`) plus `run_scene` keywords.  `f16` alone is the baseline; it always runs, and runs first.  Every mode runs every
scene with the same seed; the input latents (per VAE encode setting) and the CLIP token -- the mean embedding of the input views --
are computed once per scene.  Each (scene, mode) row holds the mean scores against the targets and `vs_baseline`, the scores
against the baseline's own frames (PSNR inf, SSIM 1 for the baseline itself).  Output: `<out>/<scene>/<mode>/` as
`scenes.write_results` writes it, `<out>/report.json` and a printed table.

Under a process group (torchrun: RANK / WORLD_SIZE / LOCAL_RANK) the windows of each run shard over the ranks as in
`pipeline.run_trajectory` and rank 0 scores and writes.  Nothing is downloaded: a weight file that is not given is an error that
names its option and its environment variable.
"""

from __future__ import annotations

import argparse
import contextlib
import json
import math
import os
import sys

import torch

from . import scenes

WEIGHTS = {"vae": "SEVA_VAE_PATH", "clip": "SEVA_CLIP_PATH", "lpips_vgg": "SEVA_LPIPS_VGG_PATH", "lpips_lin": "SEVA_LPIPS_LIN_PATH"}


# --------------------------------------------------------------------------------------------------------------- modes
def _num(tok, arg, conv=float):
    try:
        return conv(arg)
    except (TypeError, ValueError):
        raise ValueError(f"mode token {tok!r}: {arg!r} is no {conv.__name__}") from None


def _t_plain(field, key, value, needs_fp8=False):
    def apply(spec, tok, arg):
        if arg is not None:
            raise ValueError(f"mode token {tok!r} takes no '@' argument")
        spec[field][key] = value
        if needs_fp8:
            spec["_needs_fp8"].append(tok)
    return apply


def _t_dpmpp(spec, tok, arg):
    spec["run"].update(solver="dpmpp2m", num_steps=_num(tok, arg, int))


def _t_cache(spec, tok, arg):
    n, _, lv = (arg or "").partition("/")
    spec["run"]["cache_interval"] = _num(tok, n, int)
    if lv:
        spec["run"]["cache_levels"] = _num(tok, lv, int)


def _t_interval(spec, tok, arg):
    lo, sep, hi = (arg or "").partition(",")
    if not sep:
        raise ValueError(f"mode token {tok!r}: interval@lo,hi")
    spec["run"]["guidance_interval"] = (_num(tok, lo), _num(tok, hi))


def _t_rescale(spec, tok, arg):
    spec["run"]["guidance_rescale"] = _num(tok, arg)


# token -> what it sets.  "net": `Seva.set_precision` keywords; "vae": `AutoEncoder.set_precision` ("precision") / `set_upsample`
# ("upsample"); "run": `run_scene` keywords.
TOKENS = {
    "f16": _t_plain("net", "precision", "f16"),
    "fp8": _t_plain("net", "precision", "fp8"),
    "attn": _t_plain("net", "attention", "fp8", needs_fp8=True),
    "ff": _t_plain("net", "ff", "fp8", needs_fp8=True),
    "split-all": _t_plain("net", "split", "all"),
    "vae-fp8": _t_plain("vae", "precision", "fp8"),
    "vae-phases": _t_plain("vae", "upsample", "phases"),
    "dpmpp2m": _t_dpmpp,
    "cache": _t_cache,
    "interval": _t_interval,
    "rescale": _t_rescale,
}
NEEDS_ARG = ("dpmpp2m", "cache", "interval", "rescale")
BASELINE = "f16"


def parse_mode(name: str) -> dict:
    """"fp8+attn", "cache@2+vae-fp8", "interval@0.5,20" ... -> {"name", "net", "vae", "run"}; an unknown token, a missing or a
    surplus argument, or a contradiction (`attn` without `fp8`, `split-all` with `fp8`) is a ValueError."""
    spec = {"name": name, "net": {}, "vae": {}, "run": {}, "_needs_fp8": []}
    seen = set()
    for tok in name.split("+"):
        head, sep, arg = tok.partition("@")
        if head not in TOKENS:
            raise ValueError(f"unknown mode token {tok!r} in {name!r} (known: {', '.join(_known())})")
        if head in NEEDS_ARG and not sep:
            raise ValueError(f"mode token {tok!r} needs an argument: {head}@...")
        if head in seen:
            raise ValueError(f"mode {name!r}: {head!r} twice")
        seen.add(head)
        TOKENS[head](spec, tok, arg if sep else None)
    if {"f16", "fp8"} <= seen:
        raise ValueError(f"mode {name!r}: f16 and fp8 together")
    prec = spec["net"].get("precision", "f16")
    if spec.pop("_needs_fp8") and prec != "fp8":
        raise ValueError(f"mode {name!r}: attn / ff are sub-options of fp8 (fp8+attn, fp8+ff)")
    if "split" in spec["net"] and prec != "f16":
        raise ValueError(f"mode {name!r}: split-all is an f16 mode")
    return spec


def _known():
    return [t + "@..." if t in NEEDS_ARG else t for t in TOKENS]


def split_modes(text: str) -> list:
    """The --modes list: comma-separated, where the comma inside `interval@lo,hi` belongs to the token."""
    out = []
    for piece in (p.strip() for p in text.split(",")):
        last = out[-1].split("+")[-1] if out else ""
        if last.startswith("interval@") and "," not in last and _is_number(piece.split("+")[0]):
            out[-1] += "," + piece
        elif piece:
            out.append(piece)
    return out


def _is_number(s):
    try:
        float(s)
        return True
    except ValueError:
        return False


def parse_modes(text: str) -> list:
    """Mode specs of a --modes list, the baseline first (added if the list does not name it), each name once."""
    names = split_modes(text)
    names = [BASELINE] + [n for n in names if n != BASELINE]
    if len(set(names)) != len(names):
        raise ValueError(f"--modes: a mode is named twice in {names}")
    return [parse_mode(n) for n in names]


def apply_mode(spec: dict, net, ae) -> None:
    """Engine settings of a mode, set from the defaults up (a mode never inherits the one before it).  Models without the
    setter (injected stand-ins) take only modes that leave that engine alone."""
    core = getattr(net, "module", net)
    nk = {"precision": "f16", "attention": None, "ff": None, "split": None, **spec["net"]}
    if hasattr(core, "set_precision"):
        core.set_precision(nk.pop("precision"), **nk)
    elif spec["net"] and spec["net"] != {"precision": "f16"}:
        raise ValueError(f"mode {spec['name']!r} sets the network's precision; this network has no set_precision")
    if hasattr(ae, "set_precision") and hasattr(ae, "set_upsample"):
        ae.set_precision(spec["vae"].get("precision", "f16"))
        ae.set_upsample(spec["vae"].get("upsample", "taps"))
    elif spec["vae"]:
        raise ValueError(f"mode {spec['name']!r} sets the VAE; this VAE has no set_precision / set_upsample")


# ------------------------------------------------------------------------------------------------------------- running
class _EncodeInputsOnce:
    """The VAE as `run_scene` sees it during a sweep: the first `encode` after `begin(key)` is the input views' and is computed
    once per key; everything else goes to the VAE."""

    def __init__(self, ae):
        self._ae, self._cache, self._key = ae, {}, None
        self.encodes = 0

    def begin(self, key):
        self._key = key

    def encode(self, x):
        key, self._key = self._key, None
        if key is None:
            return self._ae.encode(x)
        if key not in self._cache:
            self._cache[key] = self._ae.encode(x)
            self.encodes += 1
        return self._cache[key]

    def decode(self, z):
        return self._ae.decode(z)

    def __getattr__(self, name):
        return getattr(self._ae, name)


def _size(text):
    v = [int(t) for t in str(text).replace("x", ",").split(",")]
    if len(v) not in (1, 2):
        raise ValueError(f"--size: L (shortest side) or W,H, not {text!r}")
    return v[0] if len(v) == 1 else (v[0], v[1])


def _per_pass_ints(text):
    v = [int(t) for t in str(text).split(",")]
    return v[0] if len(v) == 1 else v


def _args(argv):
    p = argparse.ArgumentParser(prog="python -m seva.evaluate", description=__doc__.split("\n\n")[0])
    p.add_argument("--scenes", required=True, help="scene folders, comma-separated")
    p.add_argument("--task", default="img2img", choices=scenes.TASKS)
    p.add_argument("--num-inputs", default=None, help="split key: a number or a string such as 3-far (default: the only split)")
    p.add_argument("--size", default="576", help="L (the reference's L_short) or W,H")
    p.add_argument("--T", default="21", help="window length, or T1,T2")
    p.add_argument("--model", default=None, help="directory holding model.safetensors")
    p.add_argument("--vae", default=None)
    p.add_argument("--clip", default=None)
    p.add_argument("--lpips-vgg", default=None)
    p.add_argument("--lpips-lin", default=None)
    p.add_argument("--modes", default=BASELINE)
    p.add_argument("--out", required=True)
    p.add_argument("--two-pass", action="store_true", help="use_traj_prior=True (img2vid / img2trajvid)")
    p.add_argument("--num-steps", type=int, default=None)
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--postprocess", default=None, help="resize:S or crop:W,H (the benchmark's image postprocessing)")
    p.add_argument("--device", default=None)
    return p.parse_args(argv)


def _weight(args, name, required=True):
    v = getattr(args, name) or os.environ.get(WEIGHTS[name])
    if not v and required:
        raise SystemExit(f"seva.evaluate: no {name.replace('_', ' ')} weights: give --{name.replace('_', '-')} or set {WEIGHTS[name]} "
                         "(a local file; nothing is downloaded)")
    if v and not os.path.exists(v):
        raise SystemExit(f"seva.evaluate: --{name.replace('_', '-')} / {WEIGHTS[name]} = {v!r}: no such file")
    return v


@contextlib.contextmanager
def _environ(**values):
    """Environment variables set for the block only."""
    before = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _load_models(args, device, net, ae, conditioner):
    """Whatever was not injected, from local files; a missing path is an error naming its option and variable."""
    lp = None
    if net is None:
        if not args.model:
            raise SystemExit("seva.evaluate: no network weights: give --model (a directory holding model.safetensors; nothing is downloaded)")
        from .utils import load_model
        net = load_model(args.model, device=device).to(device).eval()
    if ae is None:
        from .modules.autoencoder import AutoEncoder
        with _environ(SEVA_VAE_PATH=_weight(args, "vae")):  # the constructor's only way in; the variable is put back afterwards
            ae = AutoEncoder(chunk_size=1).to(device)
    if conditioner is None:
        from .modules.conditioner import CLIPConditioner
        with _environ(SEVA_CLIP_PATH=_weight(args, "clip")):
            conditioner = CLIPConditioner().to(device)
    vgg = _weight(args, "lpips_vgg", required=False)
    if vgg:
        from . import metrics
        lp = metrics.LPIPS(metrics.load_lpips_weights(vgg, _weight(args, "lpips_lin", required=False))).to(device)
    return net, ae, conditioner, lp


def _mean(rows, key, sub=None):
    vals = [(r[sub] if sub else r).get(key) for r in rows]
    vals = [v for v in vals if v is not None]
    return float(sum(vals) / len(vals)) if vals else None


def _fmt(v):
    return "      -" if v is None else ("    inf" if math.isinf(v) else f"{v:7.3f}")


def main(argv=None, *, net=None, ae=None, conditioner=None, lpips=None) -> dict | None:
    """The sweep; returns the report on rank 0 (None elsewhere).  `net` (`SGMWrapper(model)`, or any callable
    `net(x, t, cond, num_frames=)`), `ae`, `conditioner` and `lpips` take the place of the models the options would load.  Injected
    engines are set by every mode and come back at the baseline's explicit settings (`set_precision("f16")`, `set_upsample("taps")`),
    not at what they had, or took from SEVA_* variables, before the call."""
    import torch.distributed as dist
    from . import frames, metrics
    from .model import Seva, SGMWrapper
    args = _args(argv)
    specs = parse_modes(args.modes)  # before anything loads: an unknown mode costs nothing
    size, T = _size(args.size), _per_pass_ints(args.T)
    post = None
    if args.postprocess:
        kind, _, v = args.postprocess.partition(":")
        post = {kind: _size(v)}
        scenes._postprocess_size(post)
    num_inputs = args.num_inputs
    if num_inputs is not None and num_inputs.isdigit():
        num_inputs = int(num_inputs)
    tasks = [(os.path.basename(os.path.normpath(d)), scenes.read_scene(d).task(args.task, num_inputs, T))
             for d in args.scenes.split(",") if d]
    if len({n for n, _ in tasks}) != len(tasks):
        raise SystemExit("seva.evaluate: two scene folders have the same name")
    if args.two_pass and args.task == "img2img":
        raise SystemExit("seva.evaluate: img2img is one pass only")

    if "RANK" in os.environ and int(os.environ.get("WORLD_SIZE", "1")) > 1 and not dist.is_initialized():
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        dist.init_process_group("nccl")
        args.device = args.device or f"cuda:{local}"
    rank = dist.get_rank() if dist.is_initialized() else 0
    device = torch.device(args.device or "cuda")
    net, ae, conditioner, lp = _load_models(args, device, net, ae, conditioner)
    lp = lpips if lpips is not None else lp
    call = SGMWrapper(net) if isinstance(net, Seva) else net
    vae = _EncodeInputsOnce(ae)
    extra = {k: v for k, v in (("num_steps", args.num_steps), ("seed", args.seed)) if v is not None}

    rows = []
    with torch.no_grad():
        for si, (name, task) in enumerate(tasks):
            WH = task.frame_size(size)
            apply_mode(specs[0], net, ae)
            views = torch.cat([frames.load_img_and_K(task.image_paths[i], WH, device=device)[0] for i in task.input_ids])
            token = conditioner(views).mean(0)  # the reference's token of a window that conditions on the input views (eval.py:1248)
            shown = frames.to_uint8(views)  # `input/*.png` of every mode: the pictures as loaded, quantised once per scene
            base = None
            for spec in specs:
                apply_mode(spec, net, ae)
                vae.begin((si, "f16"))  # no mode changes the encode precision: one set of input latents per scene
                res = scenes.run(call, vae, task, size=WH, use_traj_prior=args.two_pass, postprocess=post, lpips=lp,
                                 clip_token=token, device=device, input_frames=shown, **{**extra, **spec["run"]})
                if rank != 0 or "frames" not in res:
                    continue
                tids = task.target_ids
                if base is None:
                    base = res["frames"][tids].clone()
                vs = metrics.compare(res["frames"][tids], base, lpips=lp)
                row = {"scene": name, "mode": spec["name"], "frames": len(tids), **scenes.metrics_table(res).get("mean", {}),
                       "vs_baseline": {k: float(vs[k].mean()) for k in ("psnr", "ssim", "lpips") if k in vs}}
                scenes.write_results(os.path.join(args.out, name, spec["name"]), res, task,
                                     options={"mode": spec["name"], "size": list(WH), "T": T, "two_pass": args.two_pass,
                                              **scenes.DEMO_DEFAULTS, "chunk_strategy": task.options["chunk_strategy"],
                                              **extra, **spec["run"]})
                rows.append(row)
    apply_mode(specs[0], net, ae)  # the engines are left at the baseline's explicit settings (f16, taps), whatever they had before
    if rank != 0:
        return None
    means = []
    for spec in specs:
        mine = [r for r in rows if r["mode"] == spec["name"]]
        means.append({"mode": spec["name"], "scenes": len(mine),
                      **{k: _mean(mine, k) for k in ("psnr", "ssim", "lpips") if _mean(mine, k) is not None},
                      "vs_baseline": {k: _mean(mine, k, "vs_baseline") for k in ("psnr", "ssim", "lpips")
                                      if _mean(mine, k, "vs_baseline") is not None}})
    report = {"task": args.task, "num_inputs": args.num_inputs, "size": args.size, "T": T, "two_pass": args.two_pass,
              "postprocess": post, "modes": [s["name"] for s in specs], "scenes": [n for n, _ in tasks],
              "input_encodes": vae.encodes, "rows": rows, "means": means}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "report.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(f"{'scene':<20}{'mode':<24}{'psnr':>8}{'ssim':>8}{'lpips':>8}  | vs baseline{'psnr':>8}{'ssim':>8}{'lpips':>8}")
    for r in rows + [{"scene": "(mean)", **m} for m in means]:
        v = r["vs_baseline"]
        print(f"{r['scene']:<20}{r['mode']:<24} {_fmt(r.get('psnr'))} {_fmt(r.get('ssim'))} {_fmt(r.get('lpips'))}  |"
              f"            {_fmt(v.get('psnr'))} {_fmt(v.get('ssim'))} {_fmt(v.get('lpips'))}")
    return report


if __name__ == "__main__":
    main(sys.argv[1:])
