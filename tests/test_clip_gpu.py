"""CLIP ViT-H-14 image conditioner on the HIP path.

The TOWER is pinned against transformers' `CLIPVisionModelWithProjection` (an independent implementation of open_clip's
vision transformer) on synthetic weights, through the fixtures tests/golden/g11_clip_*.npz (oracle/make_goldens_clip.py;
the restatement oracle/clip_ref.py meets them to < 1e-5 in tests/test_clip_parity_cpu.py).  The RESIZE -- kornia's
Gaussian antialias rule and bicubic `align_corners=True` -- remains a restatement of the published algorithm (kornia is
not available offline and the reference holds no fixture for it): the preprocess checks at sizes other than 224 are
self-consistency checks, like the VAE's."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import load_golden, rel_l2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from seva import _native
    _native.load()
    return torch.device("cuda:0")


def _conditioner(dev, params, seed=11):
    from oracle import clip_ref as CR
    from seva.modules.conditioner import CLIPConditioner
    cond = CLIPConditioner(params, random_init=True)
    shapes = CR.vit_shapes(params.width, params.layers, params.patch_size, params.image_size,
                           int(params.width * params.mlp_ratio), params.embed_dim)
    assert {k: tuple(v.shape) for k, v in cond.module.state_dict().items()} == shapes
    sd = CR.synthetic_state_dict(params, seed)
    cond.module.load_state_dict(sd, strict=True)
    return cond.to(dev), sd


@pytest.mark.parametrize("B,H,L,D", [(2, 16, 257, 80), (3, 2, 50, 64), (1, 3, 300, 128), (5, 1, 7, 2)])
def test_attention_small(dev, B, H, L, D):
    from seva import ops
    C = H * D
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B, L, 3 * C, generator=g).half().to(dev)
    out = torch.full((B, L, C), float("nan"), device=dev, dtype=torch.float16)
    ops.attention_small(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], out, batch=B, heads=H, L=L, head_dim=D,
                        q_strides=(L * 3 * C, 3 * C), k_strides=(L * 3 * C, 3 * C), o_strides=(L * C, C),
                        scale=1.0 / math.sqrt(D))
    x = qkv.view(B, L, 3, H, D).permute(2, 0, 3, 1, 4).double()
    ref = (torch.softmax(x[0] @ x[1].transpose(-1, -2) / math.sqrt(D), -1) @ x[2]).transpose(1, 2).reshape(B, L, C)
    assert torch.isfinite(out).all() and rel_l2(out, ref) < 1e-3


@pytest.mark.parametrize("n,H,W", [(2, 96, 128), (1, 576, 576), (2, 300, 224), (1, 1000, 640)])
def test_clip_preprocess_vs_restatement(dev, n, H, W):
    """up-scaling (no blur), the 576x576 case of the hot path (3x3 Gaussian), mixed, and a 7-tap blur"""
    from oracle import clip_ref as CR
    from seva.modules.conditioner import ViTParams
    cond, _ = _conditioner(dev, ViTParams(width=320, layers=1, embed_dim=64))
    x = (torch.rand(n, 3, H, W, generator=torch.Generator().manual_seed(5)) * 2 - 1)
    got = cond.preprocess(x.to(dev)).cpu()
    ref = CR.preprocess(x)
    assert got.shape == ref.shape == (n, 3, 224, 224)
    assert (got - ref).abs().max() < 4e-3 and rel_l2(got, ref) < 1e-3  # f16 storage of the patch matrix


def test_clip_tiny_tower_vs_restatement(dev):
    from oracle import clip_ref as CR
    from seva.modules.conditioner import ViTParams
    p = ViTParams(width=320, layers=3, embed_dim=128)  # 4 heads of width 80, 257 tokens
    cond, sd = _conditioner(dev, p)
    x = (torch.rand(3, 3, 160, 200, generator=torch.Generator().manual_seed(7)) * 2 - 1)
    got = cond(x.to(dev)).cpu()
    ref = CR.clip_conditioner(sd, x, heads=p.heads)
    err = rel_l2(got, ref)
    print(f"\ntiny CLIP tower (3 layers, width 320): rel-L2 {err:.3e}")
    assert got.shape == (3, 128) and err < 2e-3
    # one frame alone reproduces its row bit for bit (no cross-frame coupling anywhere)
    assert torch.equal(cond(x[1:2].to(dev)).cpu(), got[1:2])


@pytest.mark.parametrize("name", ["tiny", "wide2"])
def test_clip_tower_vs_transformers_fixture(dev, name):
    """HIP tower against the fp64 embeddings of transformers' CLIPVisionModelWithProjection (tests/golden/g11_clip_*).
    2e-3 is this file's bound for the same towers against the restatement (f16 GEMM operands); the restatement and
    transformers differ by 5e-7.  tiny: width 320, 3 layers, 3 images; wide2: ViT-H-14's widths (LayerNorm rows of 1280,
    heads of 80, K = 5120 GEMMs), 2 layers."""
    from oracle import clip_ref as CR
    from seva.modules.conditioner import ViTParams
    p = {"tiny": ViTParams(width=320, layers=3, embed_dim=128), "wide2": ViTParams(layers=2)}[name]
    g = load_golden("g11_clip_" + name)
    cond, sd = _conditioner(dev, p, int(g["seed"]))
    CR.assert_weight_sums(sd, g)
    x = g["x"].float()  # (n,3,224,224) on the grid k/128: the resize is the identity, no blur
    got = cond(x.to(dev)).cpu()
    err = rel_l2(got, g["embeds"])
    print(f"\nCLIP tower {name} vs transformers fixture: rel-L2 {err:.3e}")
    assert got.shape == g["embeds"].shape and torch.isfinite(got).all() and err < 2e-3
    mean, std = (torch.tensor(v, dtype=torch.float64)[None, :, None, None] for v in (CR.MEAN, CR.STD))
    pre = cond.preprocess(x.to(dev)).cpu()
    assert pre.shape == x.shape
    assert (pre.double() - ((x.double() + 1.0) / 2.0 - mean) / std).abs().max() < 4e-3  # f16 storage of the patch matrix
    if name == "tiny":  # one frame alone reproduces its row bit for bit
        assert torch.equal(cond(x[1:2].to(dev)).cpu(), got[1:2])


def test_clip_vit_h14_full_width(dev):
    """The real ViT-H-14 geometry (32 layers, width 1280, 16 heads x 80, MLP 5120, 1024-d output), one 576x576 frame
    against the restatement, then the 224x224 image of tests/golden/g11_clip_h14 against transformers' embeddings."""
    import time
    from oracle import clip_ref as CR
    from seva.modules.conditioner import ViTParams
    p = ViTParams()
    cond, sd = _conditioner(dev, p)
    fx = load_golden("g11_clip_h14")
    assert int(fx["seed"]) == 11
    CR.assert_weight_sums(sd, fx)
    assert sum(v.numel() for v in sd.values()) == 632_076_800
    x = (torch.rand(1, 3, 576, 576, generator=torch.Generator().manual_seed(9)) * 2 - 1)
    got = cond(x.to(dev))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = cond(x.to(dev)).cpu()
    dt = time.perf_counter() - t0
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ref = CR.clip_conditioner(sd, x, heads=p.heads)
    err = rel_l2(got, ref)
    print(f"\nCLIP ViT-H-14 (632 M params), one 576x576 frame: rel-L2 {err:.3e}; {dt * 1e3:.1f} ms per frame on the GPU")
    assert got.shape == (1, 1024) and err < 2e-3
    got_fx = cond(fx["x"].float().to(dev)).cpu()
    err_fx = rel_l2(got_fx, fx["embeds"])
    print(f"CLIP ViT-H-14 vs transformers fixture (224x224 image): rel-L2 {err_fx:.3e}")
    assert got_fx.shape == (1, 1024) and torch.isfinite(got_fx).all() and err_fx < 2e-3
