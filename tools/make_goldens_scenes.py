"""Scene-folder fixtures and what the REFERENCE makes of them (dev container only; needs the reference checkout).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens_scenes.py

tests/golden/scenes/{a_top,b_mixed,c_semidense}/   three synthetic folders in the `reconfusion` layout, written here
tests/golden/g16_scenes.json                        seva/data_io.py:330-428  ReconfusionParser (normalize=False): every field
                                                    demo.py:68-271           parse_task per (scene, task, num_inputs, T)
                                                    seva/eval.py:1355-1402   camera_cond["K"] after run_one_scene's loading loop at
                                                                             (W, H) = (64, 64), L_short = 64 and (96, 64)

The reference's modules are imported with the inert stand-ins of oracle/make_goldens_next.py (importing that module installs them
and imports the reference's `seva.eval`); `torchvision.transforms.functional.crop` / `.pad`, which the loading loop calls, are
working ones written here.  `demo.py` builds the model when it is imported, and the loading loop is the head of a function that
goes on to sample: so the `parse_task` definition, and the loop statement, are taken out of the files' syntax trees and executed in
namespaces that hold the reference functions they name.  Nothing of the reference is copied: inputs are built here, outputs are
stored as data.  Floats go to JSON through repr, which round-trips doubles; float32 results are stored as the doubles they equal.
"""

from __future__ import annotations

import ast
import copy
import json
import math
import os
import shutil
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SCENES = os.path.join(GOLD, "scenes")
sys.path.insert(0, ROOT)


# ------------------------------------------------------------------------------------------------------------ fixtures
def _orbit_gl(n, radius, height, sweep, seed):
    """OpenGL camera-to-world matrices (x right, y up, z backwards) on a jittered arc, looking at the origin."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        a = sweep * math.pi * i / n
        eye = np.array([radius * math.sin(a), height + 0.03 * i, radius * math.cos(a)]) + 0.05 * rng.standard_normal(3)
        back = eye / np.linalg.norm(eye)
        right = np.cross([0.0, 1.0, 0.0], back)
        right /= np.linalg.norm(right)
        up = np.cross(back, right)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, up, back, eye
        out.append(m)
    return np.array(out)


def _picture(w, h, seed, alpha=False):
    """A smooth gradient with a few blocks: compresses well, differs per frame."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y + 7 * seed) * 5 % 256)], -1).astype(np.uint8)
    for _ in range(3):
        x0, y0 = int(rng.integers(0, w - 6)), int(rng.integers(0, h - 6))
        img[y0:y0 + 6, x0:x0 + 6] = rng.integers(0, 256, 3, dtype=np.uint8)
    if alpha:
        a = np.full((h, w, 1), 255, np.uint8)
        a[: h // 4, : w // 4] = 96
        img = np.concatenate([img, a], -1)
    return img


def _write_scene(name, frames, top, splits, bounds=None):
    d = os.path.join(SCENES, name)
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(os.path.join(d, "images"))
    out = []
    for i, fr in enumerate(frames):
        rec = {k: v for k, v in fr.items() if k not in ("picture",)}
        if fr.get("picture") is not None:
            rel = f"images/{i:03d}.png"
            Image.fromarray(fr["picture"]).save(os.path.join(d, rel), optimize=True)
            rec["file_path"] = rel
        else:
            rec["file_path"] = None
        out.append(rec)
    with open(os.path.join(d, "transforms.json"), "w") as f:
        json.dump({**top, "frames": out}, f, indent=1)
    for key, (train, test) in splits.items():
        with open(os.path.join(d, f"train_test_split_{key}.json"), "w") as f:
            json.dump({"train_ids": train, "test_ids": test}, f)
    if bounds is not None:
        np.save(os.path.join(d, "bounds.npy"), bounds)
    return d


def make_fixtures():
    # (a) top-level intrinsics, an applied_transform (a rotation about x by 0.3 rad after a y/z swap, and a shift), splits 3 and 6
    n, w, h = 12, 48, 36
    cams = _orbit_gl(n, 2.0, 0.3, 1.2, 11)
    c, s = math.cos(0.3), math.sin(0.3)
    applied = np.array([[1, 0, 0, 0.1], [0, c, -s, -0.2], [0, s, c, 0.05]]) @ np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0], [0, 0, 0, 1.0]])
    full = np.concatenate([applied, [[0, 0, 0, 1]]], 0)
    frames = [{"transform_matrix": (full @ m).tolist(), "picture": _picture(w, h, i)} for i, m in enumerate(cams)]
    top = {"fl_x": 52.5, "fl_y": 51.75, "cx": 23.5, "cy": 18.25, "w": w, "h": h, "applied_transform": applied.tolist()}
    _write_scene("a_top", frames, top, {3: ([0, 5, 11], [1, 2, 3, 4, 6, 7, 8, 9, 10]), 6: ([0, 2, 4, 7, 9, 11], [1, 3, 5, 6, 8, 10])},
                 bounds=np.stack([np.full(n, 0.5), np.linspace(3.0, 4.0, n)], 1))
    # (b) per-frame intrinsics, landscape and portrait mixed, one target without a picture, a string split key
    n = 8
    cams = _orbit_gl(n, 1.5, 0.1, 0.8, 23)
    frames = []
    for i, m in enumerate(cams):
        w, h = (48, 32) if i % 4 < 2 else (32, 48)
        frames.append({"fl_x": 40.0 + i, "fl_y": 41.5 + 0.5 * i, "cx": w / 2 - 0.75, "cy": h / 2 + 0.5, "w": w, "h": h,
                       "transform_matrix": m.tolist(), "picture": None if i == 4 else _picture(w, h, 40 + i, alpha=i % 3 == 0)})
    _write_scene("b_mixed", frames, {}, {"2-far": ([1, 6], [0, 2, 3, 4, 5, 7])})
    # (c) 40 frames, 12 inputs: the semi-dense regime
    n, w, h = 40, 24, 24
    cams = _orbit_gl(n, 2.5, 0.2, 1.9, 37)
    frames = [{"transform_matrix": m.tolist(), "picture": _picture(w, h, 80 + i)} for i, m in enumerate(cams)]
    top = {"fl_x": 30.0, "fl_y": 30.0, "cx": 12.0, "cy": 12.0, "w": w, "h": h}
    train = [0, 3, 7, 10, 14, 17, 21, 24, 28, 31, 35, 39]
    _write_scene("c_semidense", frames, top, {12: (train, [i for i in range(n) if i not in train])})


# ----------------------------------------------------------------------------------------------------------- reference
def _tf_crop(img, top, left, height, width):
    assert 0 <= top and 0 <= left and top + height <= img.shape[-2] and left + width <= img.shape[-1]
    return img[..., top:top + height, left:left + width]


def _tf_pad(img, padding, fill=0, padding_mode="constant"):
    pl, pt, pr, pb = [int(p) for p in padding]
    return F.pad(img, (pl, pr, pt, pb), mode=padding_mode, value=fill)


def _reference():
    tv, tvt, tvf = (types.ModuleType(n) for n in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional"))
    tvf.crop, tvf.pad = _tf_crop, _tf_pad
    tv.transforms, tvt.functional = tvt, tvf
    try:
        import torchvision  # noqa: F401
    except Exception:
        sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "torchvision.transforms.functional": tvf})
    from oracle import make_goldens_next as nxt  # installs the inert stand-ins, imports the reference's seva.eval
    if "torchvision.utils" not in sys.modules:
        sys.modules["torchvision.utils"] = tv.utils = nxt._Inert("torchvision.utils")
    reval, REF = nxt.reval, nxt.REF
    if not hasattr(reval.TF, "crop") or isinstance(reval.TF, nxt._Inert):
        reval.TF = tvf
    import seva.data_io as rdata
    import seva.geometry as rgeo
    assert rdata.__file__.startswith(REF) and reval.__file__.startswith(REF)

    def definition(path, pick):
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        node = pick(tree)
        return compile(ast.Module(body=[node], type_ignores=[]), path, "exec")

    ns = {"np": np, "torch": torch, "F": F, "Image": Image, "get_parser": rdata.get_parser}
    for name in ("infer_prior_stats", "infer_prior_inds", "compute_relative_inds"):
        ns[name] = getattr(reval, name)
    for name in ("generate_interpolated_path", "generate_spiral_path", "get_arc_horizontal_w2cs", "get_default_intrinsics",
                 "get_lookat", "get_preset_pose_fov"):
        ns[name] = getattr(rgeo, name, None)
    exec(definition(os.path.join(REF, "demo.py"),
                    lambda t: next(n for n in t.body if isinstance(n, ast.FunctionDef) and n.name == "parse_task")), ns)
    loop = definition(os.path.join(REF, "seva", "eval.py"),
                      lambda t: next(s for n in t.body if isinstance(n, ast.FunctionDef) and n.name == "run_one_scene"
                                     for s in n.body if isinstance(s, ast.For)))
    return rdata, reval, ns["parse_task"], loop


def _loaded_Ks(reval, loop, paths, Ks, input_indices, W=None, H=None, L_short=None):
    """camera_cond["K"] after the loading loop of run_one_scene, run as the reference wrote it."""
    options = {} if L_short is None else {"L_short": L_short}
    ns = dict(vars(reval))
    ns.update(image_cond={"img": list(paths), "input_indices": list(input_indices)}, camera_cond={"K": Ks.clone()}, options=options,
              version_dict={"H": H, "W": W, "options": options}, W=W, H=H, F=8, imgs_clip=[], imgs=[], img_size=None, gradio=False)
    exec(loop, ns)
    assert len(ns["imgs"]) == len(paths)
    return ns["camera_cond"]["K"], [tuple(int(v) for v in im.shape[-2:]) for im in ns["imgs"]]


def _f(t):
    return np.asarray(t, dtype=np.float64).tolist()


CASES = [  # scene, task, num_inputs, T, options
    ("a_top", "img2img", 3, 21, {}), ("a_top", "img2img", 6, 21, {}), ("a_top", "img2vid", 3, 8, {}),
    ("a_top", "img2vid", 3, 8, {"chunk_strategy": "interp"}), ("a_top", "img2trajvid", 3, 8, {}),
    ("a_top", "img2trajvid", 3, 6, {"chunk_strategy": "interp-gt"}), ("a_top", "img2trajvid", 6, 9, {"chunk_strategy": "interp"}),
    ("a_top", "img2trajvid", 3, 4, {"chunk_strategy": "interp"}),
    ("b_mixed", "img2img", "2-far", 21, {}), ("b_mixed", "img2vid", "2-far", 5, {}), ("b_mixed", "img2trajvid", "2-far", 6, {}),
    ("c_semidense", "img2img", 12, 21, {}), ("c_semidense", "img2img", None, 21, {}),
    ("c_semidense", "img2trajvid", 12, [41, 21], {}), ("c_semidense", "img2trajvid", 12, [41, 21], {"chunk_strategy": "interp-gt"}),
    ("c_semidense", "img2trajvid", 12, 21, {"chunk_strategy": "interp-gt"}), ("c_semidense", "img2vid", 12, [41, 21], {}),
    ("c_semidense", "img2vid", 12, 21, {"chunk_strategy": "interp"}),
]


def main():
    if "--keep-fixtures" not in sys.argv:
        make_fixtures()
    rdata, reval, parse_task, loop = _reference()
    out = {"scenes": {}, "tasks": []}
    for name in sorted(os.listdir(SCENES)):
        d = os.path.join(SCENES, name)
        p = rdata.ReconfusionParser(d, normalize=False)
        n = len(p.image_paths)
        out["scenes"][name] = {
            "image_names": p.image_names, "image_paths": [None if q is None else os.path.relpath(q, d) for q in p.image_paths],
            "camtoworlds": _f(p.camtoworlds), "camera_ids": list(p.camera_ids), "Ks": _f([p.Ks_dict[i] for i in range(n)]),
            "imsizes": [list(p.imsize_dict[i]) for i in range(n)], "scene_scale": float(p.scene_scale),
            "transform": _f(p.transform), "bounds": None if p.bounds is None else _f(p.bounds),
            "splits": [[k, v] for k, v in p.splits_per_num_input_frames.items()]}
        print(f"{name}: {n} frames, splits {list(p.splits_per_num_input_frames)}")
    for scene, task, num_inputs, T, options in CASES:
        d = os.path.join(SCENES, scene)
        vd = {"H": 64, "W": 64, "T": copy.deepcopy(T), "C": 4, "f": 8, "options": {"chunk_strategy": "nearest-gt", **options}}
        paths, n_in, n_tgt, input_ids, anchor_indices, c2ws, Ks, anchor_c2ws, anchor_Ks = parse_task(task, d, num_inputs, vd["T"], vd)
        input_ids = [int(i) for i in input_ids]
        rec = {"scene": scene, "task": task, "num_inputs": num_inputs, "T": T, "options": options, "T_after": vd["T"],
               "image_paths": [None if q is None else os.path.relpath(q, d) for q in paths], "num_inputs_out": int(n_in),
               "num_targets": int(n_tgt), "input_indices": input_ids, "anchor_indices": [float(a) for a in anchor_indices],
               "c2ws": _f(c2ws), "Ks": _f(Ks), "anchor_ids": None}
        assert c2ws.dtype == torch.float32 and Ks.dtype == torch.float32 and c2ws.shape[1:] == (3, 4)
        if task == "img2vid":
            rec["anchor_ids"] = [int(a) for a in anchor_indices]
        elif task == "img2trajvid":
            rec["anchor_ids"] = [int(n_in + j) for j in np.linspace(0, n_tgt - 1, len(anchor_indices)).round().astype(np.int64)]
        if rec["anchor_ids"] is not None:  # the anchors the reference hands to run_one_scene are these trajectory frames
            assert torch.equal(anchor_c2ws, c2ws[rec["anchor_ids"]]) and torch.equal(anchor_Ks, Ks[rec["anchor_ids"]])
        else:
            assert anchor_c2ws is None and anchor_Ks is None
        rec["Ks_at"] = {}
        for tag, kw in (("64x64", dict(W=64, H=64)), ("L64", dict(L_short=64)), ("96x64", dict(W=96, H=64))):
            K, hw = _loaded_Ks(reval, loop, paths, Ks, input_ids, **kw)
            assert K.dtype == torch.float32
            rec["Ks_at"][tag] = {"Ks": _f(K), "frame_hw": [list(v) for v in hw]}
        out["tasks"].append(rec)
        print(f"{scene} {task} num_inputs={num_inputs} T={T} {options}: {n_in} in, {n_tgt} targets, anchors {rec['anchor_ids']}, T -> {vd['T']}")
    path = os.path.join(GOLD, "g16_scenes.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(f"g16_scenes.json: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
