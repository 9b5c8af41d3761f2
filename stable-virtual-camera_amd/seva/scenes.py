"""Scene folders in, scored results out: the layer between a benchmark split on disk and `pipeline.run_scene`.

    read_scene(path) -> Scene            the reference's `ReconfusionParser` (seva/data_io.py:330-428, normalize=False): `transforms.json`,
                                         every `train_test_split_<key>.json`, `bounds.npy`
    Scene.task(...) -> SceneTask         the reference's `parse_task` (demo.py:120-259) for img2img / img2vid / img2trajvid: frame order,
                                         input ids, target ids and the frame ids of its anchors
    SceneTask.Ks(size)                   the intrinsics that reach the sampler: the reference's `camera_cond["K"]` after the loop at
                                         seva/eval.py:1355-1402, through the host rules of `seva.frames` (no pixel is touched)
    run(net, ae, task, ...)              `pipeline.run_scene` on the task's pictures, cameras and anchors, with the demo's sampling defaults
    write_results(dir, res, task)        PNG frames, `transforms.json` (a scene folder again) and `metrics.json`

Nothing here computes on a picture- or latent-sized tensor: pictures are loaded, resized, quantised and scored by `seva.frames` and
`seva.metrics`; encode, sample and decode are `pipeline.run_scene`'s.  The host's share is JSON, 4 x 4 and 3 x 3 matrices, and PNG
compression (PIL).  Not covered: the single-image task `img2trajvid_s-prob` and the camera presets, virtual anchors that are not
trajectory frames (`traj_prior` for img2img), the COLMAP parser, video files.
"""

from __future__ import annotations

import glob
import json
import os
from dataclasses import dataclass, field

import numpy as np
import torch

from . import frames, planner

TASKS = ("img2img", "img2vid", "img2trajvid")
L_SHORT_STRIDE = 64  # eval.py:1376-1385: F * 2**downsample = 8 * 8

# demo.py:293-305, under the names `pipeline.run_trajectory` gives them
DEMO_DEFAULTS = dict(chunk_strategy="nearest-gt", guider=1, cfg=2.0, camera_scale=2.0, num_steps=50, cfg_min=1.2, seed=23)


class SceneError(ValueError):
    """A scene folder or a task request that cannot be read as asked; the message names the file and the key."""


def _json(path: str):
    try:
        with open(path) as f:
            return json.load(f)
    except FileNotFoundError:
        raise SceneError(f"{path}: no such file") from None
    except json.JSONDecodeError as e:
        raise SceneError(f"{path}: not JSON ({e})") from None


def _split_key(path: str):
    key = os.path.basename(path).split("_")[-1].removesuffix(".json")
    return int(key) if key.isdigit() else key


@dataclass
class Scene:
    """What the folder says, frame by frame in file order.  `c2ws`: OpenCV camera-to-world, float64; `Ks`: pixel intrinsics of the
    source pictures, float64; `sizes`: (w, h) as the file states them; `splits`: {key: {"train_ids", "test_ids"}}."""
    path: str
    image_paths: list
    image_names: list
    c2ws: np.ndarray
    Ks: np.ndarray
    sizes: list
    splits: dict
    bounds: np.ndarray | None = None
    _picture_sizes: dict = field(default_factory=dict, repr=False)

    def __len__(self) -> int:
        return len(self.image_paths)

    def picture_size(self, i: int):
        """(w, h) of frame i's picture as PIL reads its header (the reference sizes a frame by the picture it opened, not by the
        file's `w` / `h`); None for a frame without a picture."""
        p = self.image_paths[i]
        if p is None:
            return None
        if i not in self._picture_sizes:
            from PIL import Image
            try:
                with Image.open(p) as im:
                    self._picture_sizes[i] = tuple(int(v) for v in im.size)
            except FileNotFoundError:
                raise SceneError(f"{p}: no such picture (frame {i} of {os.path.join(self.path, 'transforms.json')})") from None
        return self._picture_sizes[i]

    def task(self, task: str, num_inputs=None, T=21, options: dict | None = None) -> "SceneTask":
        return _task(self, task, num_inputs, T, options)


def read_scene(path: str) -> Scene:
    """A folder in the `reconfusion` layout -> `Scene`.  Intrinsics and size: the file's top level, else the frame's own.  An
    `applied_transform` is undone (float64), cameras go from OpenGL to OpenCV (columns 1 and 2 negated), `file_path: null` is a frame
    without a picture."""
    path = os.fspath(path)
    tf = os.path.join(path, "transforms.json")
    meta = _json(tf)
    if not isinstance(meta, dict) or "frames" not in meta:
        raise SceneError(f"{tf}: no 'frames'")
    splits = {}
    for p in sorted(glob.glob(os.path.join(path, "train_test_split_*.json"))):
        d = _json(p)
        for k in ("train_ids", "test_ids"):
            if not isinstance(d, dict) or k not in d:
                raise SceneError(f"{p}: no '{k}'")
        splits[_split_key(p)] = {"train_ids": [int(i) for i in d["train_ids"]], "test_ids": [int(i) for i in d["test_ids"]]}
    undo = None
    if "applied_transform" in meta:
        undo = np.linalg.inv(np.concatenate([meta["applied_transform"], [[0, 0, 0, 1]]], axis=0))
    paths, names, cams, Ks, sizes = [], [], [], [], []
    for i, fr in enumerate(meta["frames"]):
        for k in ("file_path", "transform_matrix"):
            if k not in fr:
                raise SceneError(f"{tf}: frame {i} has no '{k}'")
        v = {}
        for k in ("fl_x", "fl_y", "cx", "cy", "w", "h"):
            v[k] = meta.get(k, fr.get(k, None))
            if v[k] is None:
                raise SceneError(f"{tf}: no '{k}', neither at the top level nor in frame {i}")
        p = None if fr["file_path"] is None else os.path.join(path, fr["file_path"])
        paths.append(p)
        names.append(None if p is None else os.path.basename(p))
        cam = np.array(fr["transform_matrix"])
        if cam.shape != (4, 4):
            raise SceneError(f"{tf}: 'transform_matrix' of frame {i} is {cam.shape}, not (4, 4)")
        cams.append(cam if undo is None else undo @ cam)
        Ks.append(np.array([[v["fl_x"], 0.0, v["cx"]], [0.0, v["fl_y"], v["cy"]], [0.0, 0.0, 1.0]]))
        sizes.append((v["w"], v["h"]))
    for key, d in splits.items():
        bad = [i for i in d["train_ids"] + d["test_ids"] if not 0 <= i < len(paths)]
        if bad:
            raise SceneError(f"{os.path.join(path, f'train_test_split_{key}.json')}: ids {bad} outside the {len(paths)} frames")
    c2ws = np.array(cams, dtype=np.float64).reshape(-1, 4, 4)
    c2ws[:, :, [1, 2]] *= -1
    bounds = None
    if os.path.exists(os.path.join(path, "bounds.npy")):
        bounds = np.load(os.path.join(path, "bounds.npy"), allow_pickle=False)
    return Scene(path, paths, names, c2ws, np.array(Ks, dtype=np.float64).reshape(-1, 3, 3), sizes, splits, bounds)


@dataclass
class SceneTask:
    """One task on one scene, frames in the task's order (ids below index that order; `scene_ids` maps them to the file's).
    `c2ws` (n,4,4) / `Ks_px` (n,3,3): float32, cast once from the scene's float64; `Ks_px` are the SOURCE pictures' pixel intrinsics.
    `anchor_ids`: frame ids of the reference's anchors, None for img2img (one pass only).  `T` is the request; `T_passes` what
    `infer_prior_stats` makes of it (a pair from nine inputs on).  `anchor_indices` is `parse_task`'s own list, kept as a record."""
    task: str
    scene: Scene
    scene_ids: list
    image_paths: list
    num_inputs: int
    num_targets: int
    input_ids: list
    target_ids: list
    anchor_ids: list | None
    anchor_indices: list
    c2ws: torch.Tensor
    Ks_px: torch.Tensor
    T: object
    T_passes: object
    options: dict

    def picture_sizes(self) -> list:
        """Per frame (w, h) of its picture; a frame without one takes the size of the last frame before it that had one
        (eval.py:1357: `img or img_size`)."""
        out, last = [], None
        for j, sid in enumerate(self.scene_ids):
            wh = self.scene.picture_size(sid)
            if wh is None:
                if last is None:
                    raise SceneError(f"{self.scene.path}: frame {sid} has no picture and no frame before it has one to take the size from")
                wh = last
            out.append(wh)
            last = wh
        return out

    def _plans(self, size):
        stride = 1 if isinstance(size, (tuple, list)) else L_SHORT_STRIDE
        return [(frames.plan_load(h, w, None), frames.plan_transform(h, w, size, size_stride=stride), h, w)
                for w, h in self.picture_sizes()]

    def frame_size(self, size) -> tuple:
        """(W, H) of the frames at `size`: the pair itself, or what the reference's `L_short` (an int: shortest side, rounded to a
        multiple of 64) makes of the pictures, which must then agree on it."""
        if isinstance(size, (tuple, list)):
            return int(size[0]), int(size[1])
        whs = sorted({(p.W, p.H) for _, p, _, _ in self._plans(size)})
        if len(whs) != 1:
            raise SceneError(f"{self.scene.path}: L_short = {size} gives frames of different sizes {whs}; give size=(W, H)")
        return whs[0]

    def Ks_pixels(self, size) -> torch.Tensor:
        """(n,3,3) float32: every frame's intrinsics after the cover-and-crop of ITS picture to `size`, in pixels of the frame."""
        out = []
        for K, (p0, p, h, w) in zip(self.Ks_px, self._plans(size)):
            K = frames.adjust_K(K, p0, h, w, shift=(-p0.cl, -p0.ct))  # load at the source size (eval.py:1357)
            out.append(frames.adjust_K(K[None], p, h, w)[0])           # cover and crop (eval.py:1360-1396)
        return torch.stack(out)

    def Ks(self, size) -> torch.Tensor:
        """(n,3,3) float32, what reaches the sampler: `Ks_pixels` with row 0 divided by the frame's W and row 1 by its H
        (eval.py:1399-1402).  Under `L_short` every frame is divided by its own size."""
        Ks = self.Ks_pixels(size)
        for K, (_, p, _, _) in zip(Ks, self._plans(size)):
            K[0] /= p.W
            K[1] /= p.H
        return Ks


def _task(scene: Scene, task: str, num_inputs, T, options) -> SceneTask:
    if task not in TASKS:
        raise SceneError(f"unknown task {task!r} ({' | '.join(TASKS)})")
    where = os.path.join(scene.path, "train_test_split_*.json")
    if not scene.splits:
        raise SceneError(f"{where}: the scene has no split; a task needs one")
    if num_inputs is None:
        if len(scene.splits) != 1:
            raise SceneError(f"{where}: {len(scene.splits)} splits ({sorted(scene.splits, key=str)}); say which with num_inputs=")
        num_inputs = next(iter(scene.splits))
    if num_inputs not in scene.splits:
        raise SceneError(f"{where}: no split {num_inputs!r} (there: {sorted(scene.splits, key=str)})")
    split = scene.splits[num_inputs]
    if isinstance(num_inputs, str):
        num_inputs = int(num_inputs.split("-")[0])
    train, test = list(split["train_ids"]), list(split["test_ids"])
    opts = {"chunk_strategy": DEMO_DEFAULTS["chunk_strategy"], **(options or {})}
    T = [int(t) for t in T] if isinstance(T, (list, tuple)) else int(T)
    vd = {"T": T, "options": opts}
    num_targets = len(test)
    anchor_ids = None
    if task == "img2img":
        n_anchor = planner.infer_prior_stats(T, num_inputs, num_targets, vd)
        order = np.sort(np.array(train + test))
        if len(order) <= 2:
            raise SceneError(f"{where}: img2img needs more than two frames")
        ids = [int(i) for i in order]
        input_ids = [int(i) for i in planner.compute_relative_inds(order, np.array(train))]
        anchor_indices = np.arange(len(ids), len(ids) + n_anchor).tolist()
    elif task == "img2vid":
        ids = list(range(len(scene)))
        num_targets = len(ids) - num_inputs
        n_anchor = planner.infer_prior_stats(T, num_inputs, num_targets, vd)
        input_ids = train
        anchor_indices = planner.infer_prior_inds(scene.c2ws, n_anchor, input_ids, opts).tolist()
        anchor_ids = [int(a) for a in anchor_indices]
    else:
        n_anchor = planner.infer_prior_stats(T, num_inputs, num_targets, vd)
        ids = train + test
        input_ids = np.arange(num_inputs).tolist()
        pick = np.linspace(0, num_targets - 1, n_anchor).round().astype(np.int64)
        anchor_ids = [int(num_inputs + j) for j in pick]
        anchor_indices = np.linspace(num_inputs, num_inputs + num_targets - 1, n_anchor).tolist()
    target_ids = [i for i in range(len(ids)) if i not in set(input_ids)]
    return SceneTask(task, scene, ids, [scene.image_paths[i] for i in ids], num_inputs, num_targets, input_ids, target_ids,
                     anchor_ids, anchor_indices, torch.tensor(scene.c2ws[ids]).float(), torch.tensor(scene.Ks[ids]).float(),
                     T, vd["T"], opts)


def _postprocess_size(postprocess):
    if postprocess is None:
        return None
    if not (isinstance(postprocess, dict) and len(postprocess) == 1 and next(iter(postprocess)) in ("resize", "crop")):
        raise ValueError(f'postprocess: {{"resize": s}} or {{"crop": (W, H)}}, not {postprocess!r}')
    (kind, v), = postprocess.items()
    if kind == "resize":
        return int(v)
    return int(v[0]), int(v[1])


def run(net, ae, task: SceneTask, *, size, use_traj_prior: bool, postprocess: dict | None = None, lpips=None,
        input_frames: torch.Tensor | None = None, **kw) -> dict:
    """`pipeline.run_scene` on a `SceneTask`: the input views' paths as `images`, every target frame that has a picture as a
    `targets` entry, the task's `Ks(size)`, its `anchor_ids` (two passes) and the demo's sampling defaults (`DEMO_DEFAULTS`; `T`,
    `options` and with them the chunk strategy from the task: a `chunk_strategy=` that contradicts the task raises); `kw` overrides
    the others and carries everything else `run_scene` takes (`clip_token=` or `conditioner=`,
    `device=`, the opt-in modes).  `size`: (W, H), or an int for the reference's `L_short`.
    `postprocess`: the benchmark's "Image Postprocessing" column, applied to generated frames and targets alike before scoring --
    {"resize": s} brings the shorter side to s, {"crop": (W, H)} covers and centre-crops -- through `frames.transform_img_and_K`
    (this package's area resize; the reference names no filter) and `frames.to_uint8`.  The frames in the result stay as sampled.
    On rank 0 the result of `run_scene` plus "input_frames" (n_in,H,W,3) uint8, the input pictures as loaded, and "size".
    `input_frames=`: those pictures where the caller has them already (a sweep loads them once per scene); else they are loaded here."""
    from . import metrics, pipeline
    post = _postprocess_size(postprocess)
    if use_traj_prior and task.anchor_ids is None:
        raise SceneError(f"task {task.task!r} is one pass only (its anchors are no trajectory frames): use_traj_prior=False")
    W, H = task.frame_size(size)
    Ks = task.Ks(size)
    Ks_in = Ks.clone()
    Ks_in[task.input_ids] = task.Ks_px[task.input_ids]  # `run_scene` adjusts the input views' pixel intrinsics by the same host rules
    images = [task.image_paths[i] for i in task.input_ids]
    if any(p is None for p in images):
        raise SceneError(f"{task.scene.path}: an input view has no picture")
    targets = {i: task.image_paths[i] for i in task.target_ids if task.image_paths[i] is not None}
    # one source for the chunk strategy, as in the reference (`options["chunk_strategy"]` is read by parse_task and by run_one_scene):
    # the one the task's anchors and window lengths were inferred under
    strategy = task.options["chunk_strategy"]
    for where, got in (("chunk_strategy=", kw.get("chunk_strategy")), ("options=", (kw.get("options") or {}).get("chunk_strategy"))):
        if got is not None and got != strategy:
            raise SceneError(f"{where} asks for chunk strategy {got!r}, but the task was stated under {strategy!r} "
                             f"(its anchors and window lengths follow it): state the task with options={{'chunk_strategy': {got!r}}}")
    args = {**DEMO_DEFAULTS, "T": task.T, **kw, "chunk_strategy": strategy, "options": {**task.options, **(kw.get("options") or {})}}
    if use_traj_prior:
        args.setdefault("anchor_ids", task.anchor_ids)
    else:
        args.setdefault("task", task.task)
    own = post is None
    res = pipeline.run_scene(net, ae, images, task.c2ws, Ks_in, task.input_ids, size=(W, H), use_traj_prior=use_traj_prior,
                             targets=targets if own else None, lpips=lpips if own else None, **args)
    if "frames" not in res:  # not rank 0
        return res
    dev = res["frames"].device
    if not torch.equal(res["Ks"].cpu() / res["Ks"].new_tensor([W, H, 1.0]).cpu()[:, None], Ks[task.input_ids]):
        raise AssertionError("the input views' intrinsics that were sampled are not the task's")
    res["size"] = (W, H)
    if input_frames is None:
        input_frames = torch.cat([frames.to_uint8(frames.load_img_and_K(p, (W, H), device=dev)[0]) for p in images])
    if tuple(input_frames.shape) != (len(images), H, W, 3) or input_frames.dtype != torch.uint8:
        raise ValueError(f"input_frames: ({len(images)}, {H}, {W}, 3) uint8, not {tuple(input_frames.shape)} {input_frames.dtype}")
    res["input_frames"] = input_frames
    if not own and targets:
        tids = sorted(targets)
        want = torch.cat([frames.load_img_and_K(targets[f], (W, H), device=dev)[0] for f in tids])
        got = frames.to_uint8(frames.transform_img_and_K(res["rgb"][tids], post)[0])
        want = frames.to_uint8(frames.transform_img_and_K(want, post)[0])
        m = metrics.compare(got, want, lpips=lpips)
        res["metrics"] = {"frame_ids": tids, "sse": m["sse"], "psnr": m["psnr"], "ssim": m["ssim"]}
        if lpips is not None:
            res["metrics"]["lpips"] = m["lpips"]
    if postprocess is not None:
        res["postprocess"] = dict(postprocess)
    return res


def metrics_table(res: dict) -> dict:
    """The "metrics" of a result as plain lists and means: {"frame_ids", "psnr", "ssim", ["lpips"], "mean": {...}}.  A mean over
    frames that holds an infinite PSNR is infinite."""
    m = res.get("metrics")
    if not m:
        return {}
    out = {"frame_ids": [int(i) for i in m["frame_ids"]], "mean": {}}
    for k in ("psnr", "ssim", "lpips"):
        if k in m:
            out[k] = [float(v) for v in m[k].tolist()]
            out["mean"][k] = float(sum(out[k]) / len(out[k]))
    return out


def write_results(out_dir: str, res: dict, task: SceneTask, options: dict | None = None) -> dict:
    """A result of `run` -> a folder: `input/%03d.png` (the input pictures as loaded, in `input_ids` order), `samples-rgb/%03d.png`
    (the generated frames, in `target_ids` order), `transforms.json` in `create_transforms_simple`'s schema (eval.py:1010-1034:
    OpenGL cameras, fl_x, fl_y, cx, cy, w, h, a relative file_path) and `metrics.json` (per-frame and mean psnr / ssim / lpips, the
    frame ids, `options`).  Where the reference pairs the SOURCE pictures' intrinsics with the frames' width and height
    (demo.py:395-403), this file holds the intrinsics of the saved frames, in pixels: `read_scene(out_dir)` returns the cameras that
    were sampled.  Also `train_test_split_<num_inputs>.json`, so that the folder can be stated as a task again; split files of earlier
    results in the same folder are removed first, a result folder has one split.  The split holds the ids of the task's own frame
    order (the order of `transforms.json` here): read back, img2trajvid gives the same task (train ids first, then test ids);
    img2img and img2vid results read back as img2img / img2vid keep their order, but as img2trajvid the inputs come first.
    Returns what went into `metrics.json`."""
    from PIL import Image
    out_dir = os.fspath(out_dir)
    fr = res["frames"].cpu().numpy()
    n, H, W, _ = fr.shape
    assert n == len(task.scene_ids), "the result is not this task's"
    inp = res["input_frames"].cpu().numpy()
    rel = {}
    for sub, ids, arr in (("input", task.input_ids, inp), ("samples-rgb", task.target_ids, fr[task.target_ids])):
        os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
        for j, (fid, img) in enumerate(zip(ids, arr)):
            rel[fid] = f"./{sub}/{j:03d}.png"
            Image.fromarray(np.ascontiguousarray(img)).save(os.path.join(out_dir, sub, f"{j:03d}.png"))
    Ks = task.Ks_pixels((W, H))
    gl = task.c2ws.double() @ torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0], dtype=torch.float64))
    out_frames = [{"fl_x": K[0][0].item(), "fl_y": K[1][1].item(), "cx": K[0][2].item(), "cy": K[1][2].item(), "w": W, "h": H,
                   "file_path": rel[i], "transform_matrix": gl[i].tolist()} for i, K in enumerate(Ks)]
    with open(os.path.join(out_dir, "transforms.json"), "w") as f:
        json.dump({"orientation_override": "none", "frames": out_frames}, f, indent=5)
    for stale in glob.glob(os.path.join(out_dir, "train_test_split_*.json")):
        os.remove(stale)
    with open(os.path.join(out_dir, f"train_test_split_{task.num_inputs}.json"), "w") as f:
        json.dump({"train_ids": list(task.input_ids), "test_ids": list(task.target_ids)}, f)
    rec = {"task": task.task, "scene": task.scene.path, "size": [W, H], "scene_ids": [int(i) for i in task.scene_ids],
           "input_ids": [int(i) for i in task.input_ids], "target_ids": [int(i) for i in task.target_ids],
           "anchor_ids": task.anchor_ids, "options": options or {}, **metrics_table(res)}
    if "postprocess" in res:
        rec["postprocess"] = res["postprocess"]
    with open(os.path.join(out_dir, "metrics.json"), "w") as f:
        json.dump(rec, f, indent=1, default=_jsonable)
    return rec


def _jsonable(v):
    if isinstance(v, (np.integer, np.floating)):
        return v.item()
    if isinstance(v, (np.ndarray, torch.Tensor)):
        return v.tolist()
    if isinstance(v, (tuple, set)):
        return list(v)
    return str(v)
