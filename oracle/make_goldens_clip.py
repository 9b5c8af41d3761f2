"""TEST INFRASTRUCTURE -- fixtures that pin the CLIP vision tower against an independent implementation (CPU only).

    PYTHONDONTWRITEBYTECODE=1 python oracle/make_goldens_clip.py            # write tests/golden/g11_clip_*.npz
    PYTHONDONTWRITEBYTECODE=1 python oracle/make_goldens_clip.py --check    # recompute and compare with the committed files

open_clip is not installed, but `transformers` is, and its `CLIPVisionModelWithProjection` is a separately written,
widely used implementation of the same network (the laion ViT-H-14 checkpoint is published in that format too, with
`hidden_act="gelu"`).  The model is built from a config alone -- nothing is fetched, no hub name is ever passed -- and
loaded, strictly, with the synthetic open_clip-named weights of `oracle/clip_ref.py::synthetic_state_dict` through the
key map below; it runs in fp64.  What is stored is data: the input image, the embeddings, and what is needed to tell
a drift of the seeded weights from a parity failure.

g11_clip_tiny    width  320,  3 layers,  4 heads x 80, MLP 1280, embed  128, n = 3
g11_clip_wide2   width 1280,  2 layers, 16 heads x 80, MLP 5120, embed 1024, n = 1   (ViT-H-14's row / head / K widths)
g11_clip_h14     width 1280, 32 layers, 16 heads x 80, MLP 5120, embed 1024, n = 1   (full ViT-H-14, wide2's image)

The images are 224 x 224 already: the antialias blur applies only when down-scaling and a bicubic `align_corners=True`
resize to the same size is the identity, so the fixtures do not depend on the restated kornia resize.  They lie on the
grid k/128 in [-1, 1], exact in float16.
"""

from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
for _p in (ROOT, os.path.join(ROOT, "stable-virtual-camera_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import clip_ref as CR  # noqa: E402
from seva.modules.conditioner import ViTParams  # noqa: E402

SEED = 11
RULE = ("pixel_values = ((x + 1) / 2 - mean) / std per channel, in float64, mean = (0.48145466, 0.4578275, 0.40821073), "
        "std = (0.26862954, 0.26130258, 0.27577711); x is (n,3,224,224) in [-1,1], already at the tower's size")
# name -> (tower, number of images, image seed); wide2 and h14 share one image
GEOMETRIES = {
    "g11_clip_tiny": (ViTParams(width=320, layers=3, embed_dim=128), 3, 101),
    "g11_clip_wide2": (ViTParams(layers=2), 1, 102),
    "g11_clip_h14": (ViTParams(), 1, 102),
}


def make_image(n: int, seed: int) -> torch.Tensor:
    """(n,3,224,224) on the grid k/128, k in [-128, 128]: exact in float16."""
    k = torch.randint(-128, 129, (n, 3, 224, 224), generator=torch.Generator().manual_seed(seed))
    return (k.double() / 128.0).half()


def pixel_values(x: torch.Tensor) -> torch.Tensor:
    """RULE, in float64."""
    mean = torch.tensor(CR.MEAN, dtype=torch.float64)[None, :, None, None]
    std = torch.tensor(CR.STD, dtype=torch.float64)[None, :, None, None]
    return ((x.double() + 1.0) / 2.0 - mean) / std


def to_transformers_keys(sd: dict) -> dict:
    """open_clip `visual.*` state_dict -> `CLIPVisionModelWithProjection` state_dict."""
    vm = "vision_model."
    out = {
        vm + "embeddings.class_embedding": sd["visual.class_embedding"],
        vm + "embeddings.position_embedding.weight": sd["visual.positional_embedding"],
        vm + "embeddings.patch_embedding.weight": sd["visual.conv1.weight"],
        "visual_projection.weight": sd["visual.proj"].T.contiguous(),
    }
    for wb in ("weight", "bias"):
        out[vm + "pre_layrnorm." + wb] = sd["visual.ln_pre." + wb]  # (sic)
        out[vm + "post_layernorm." + wb] = sd["visual.ln_post." + wb]
    i = 0
    while f"visual.transformer.resblocks.{i}.ln_1.weight" in sd:
        b, e = f"visual.transformer.resblocks.{i}.", vm + f"encoder.layers.{i}."
        width = sd[b + "attn.in_proj_bias"].shape[0] // 3
        for wb in ("weight", "bias"):
            for j, name in enumerate(("q_proj", "k_proj", "v_proj")):  # row thirds of the fused projection
                out[e + f"self_attn.{name}.{wb}"] = sd[b + "attn.in_proj_" + wb][j * width:(j + 1) * width].clone()
            out[e + "self_attn.out_proj." + wb] = sd[b + "attn.out_proj." + wb]
            out[e + "layer_norm1." + wb] = sd[b + "ln_1." + wb]
            out[e + "layer_norm2." + wb] = sd[b + "ln_2." + wb]
            out[e + "mlp.fc1." + wb] = sd[b + "mlp.c_fc." + wb]
            out[e + "mlp.fc2." + wb] = sd[b + "mlp.c_proj." + wb]
        i += 1
    return out


def build_model(p, sd: dict):
    """transformers' vision tower with projection, from a config alone, fp64, eager attention, loaded strictly."""
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    cfg = CLIPVisionConfig(hidden_size=p.width, intermediate_size=int(p.width * p.mlp_ratio), projection_dim=p.embed_dim,
                           num_hidden_layers=p.layers, num_attention_heads=p.heads, image_size=p.image_size,
                           patch_size=p.patch_size, hidden_act="gelu", layer_norm_eps=1e-5, attention_dropout=0.0)
    cfg._attn_implementation = "eager"
    model = CLIPVisionModelWithProjection(cfg).double()
    model.load_state_dict({k: v.double() for k, v in to_transformers_keys(sd).items()}, strict=True)
    if model.config._attn_implementation != "eager":
        raise RuntimeError("transformers did not keep the eager attention")
    return model.eval()


def reference_embeds(p, sd: dict, x: torch.Tensor) -> torch.Tensor:
    """float64 (n, embed) image embeddings of transformers' model for the image x (float16, [-1,1])."""
    model = build_model(p, sd)
    with torch.no_grad():
        out = model(pixel_values=pixel_values(x)).image_embeds
    assert out.dtype == torch.float64
    return out


def compute(name: str) -> dict:
    import transformers
    p, n, img_seed = GEOMETRIES[name]
    sd = CR.synthetic_state_dict(p, SEED)
    x = make_image(n, img_seed)
    emb = reference_embeds(p, sd, x)
    with torch.no_grad():
        o32 = CR.encode_image(sd, pixel_values(x).float(), p.heads, p.patch_size)
        o32p = CR.clip_conditioner(sd, x.float(), p.heads, p.patch_size, p.image_size)
    rel = lambda a: float((a.double() - emb).norm() / emb.norm())
    print(f"{name}: restatement fp32 vs transformers fp64: encode_image {rel(o32):.3e}, clip_conditioner {rel(o32p):.3e}")
    out = {"x": x.numpy(), "embeds": emb.numpy(), "seed": np.int64(SEED), "pixel_values_rule": np.str_(RULE),
           "transformers_version": np.str_(transformers.__version__), "torch_version": np.str_(torch.__version__)}
    out.update({k: np.float64(v) for k, v in CR.weight_sums(sd).items()})
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="recompute every fixture and compare with the committed file")
    ap.add_argument("--only", choices=sorted(GEOMETRIES), default=None)
    args = ap.parse_args()
    bad = 0
    for name in ([args.only] if args.only else GEOMETRIES):
        new = compute(name)
        path = os.path.join(GOLD, name + ".npz")
        if not args.check:
            np.savez_compressed(path, **new)
            print(f"wrote {path}: {os.path.getsize(path)} bytes")
            continue
        old = np.load(path, allow_pickle=False)
        same_x = np.array_equal(old["x"], new["x"]) and old["x"].dtype == np.float16
        sums = all(float(old[k]) == float(new[k]) for k in ("wsum_conv1", "wsum_c_proj", "wsum_proj"))
        d = float(np.linalg.norm(old["embeds"] - new["embeds"]) / np.linalg.norm(old["embeds"]))
        ok = same_x and sums and int(old["seed"]) == SEED and str(old["pixel_values_rule"]) == RULE and d <= 1e-12
        print(f"check {name}: image equal {same_x}, weight sums equal {sums}, embeds rel-L2 to the committed file {d:.3e}"
              f" (made with transformers {old['transformers_version']}, torch {old['torch_version']}): "
              f"{'ok' if ok else 'MISMATCH'}")
        bad += not ok
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
