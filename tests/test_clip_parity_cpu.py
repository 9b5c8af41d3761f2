"""The CLIP vision tower against transformers' `CLIPVisionModelWithProjection`, through fixtures (CPU).

tests/golden/g11_clip_{tiny,wide2,h14}.npz hold, for synthetic open_clip-named weights (oracle/clip_ref.py::
synthetic_state_dict), the fp64 embeddings of transformers' independently written implementation of the network
(oracle/make_goldens_clip.py).  Checked here: the restatement oracle/clip_ref.py (the reference of the HIP tests) and
the host logic of seva/_clip_engine.py.  The tight bound sits on the restatement, in fp32 on the CPU, because the
f16-operand bound of the HIP path (2e-3) could not see, say, a tanh-GELU (1.6e-4); tests/test_clip_gpu.py ties the HIP
path to the same fixtures.  The inputs are 224 x 224, so the restated kornia resize (an identity there) is NOT pinned
by any of this.
"""
import types

import pytest
import torch
import torch.nn.functional as F

import fake_ops
from conftest import load_golden, rel_l2

BOUND = 1e-5  # ~20x the fp32 rounding of the restatement measured below, 16x below the nearest wrong variant (tanh-GELU)


def tower_params(name):
    from seva.modules.conditioner import ViTParams
    return {"tiny": ViTParams(width=320, layers=3, embed_dim=128), "wide2": ViTParams(layers=2), "h14": ViTParams()}[name]


def pixel_values(x):
    """The fixtures' `pixel_values_rule`, in float64."""
    from oracle import clip_ref as CR
    mean = torch.tensor(CR.MEAN, dtype=torch.float64)[None, :, None, None]
    std = torch.tensor(CR.STD, dtype=torch.float64)[None, :, None, None]
    return ((x.double() + 1.0) / 2.0 - mean) / std


def load_tower(name):
    """(fixture, params, state dict); the stored weight sums are asserted before anything is compared."""
    from oracle import clip_ref as CR
    g = load_golden("g11_clip_" + name)
    p = tower_params(name)
    sd = CR.synthetic_state_dict(p, int(g["seed"]))
    CR.assert_weight_sums(sd, g)
    assert g["x"].dtype == torch.float16 and g["embeds"].dtype == torch.float64
    assert tuple(g["x"].shape[1:]) == (3, 224, 224) and tuple(g["embeds"].shape) == (g["x"].shape[0], p.embed_dim)
    return g, p, sd


@pytest.fixture(scope="module")
def towers():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = load_tower(name)
        return cache[name]

    yield get
    cache.clear()


@pytest.mark.parametrize("name", ["tiny", "wide2", "h14"])
def test_restatement_vs_transformers_fixture(towers, name):
    """oracle/clip_ref.py in fp32 against transformers in fp64, rel-L2 < 1e-5.  Measured when the fixtures were made
    (encode_image on the fixture's pixel values / clip_conditioner with the oracle's own preprocess in front):
    tiny 5.4e-7 / 5.5e-7, wide2 4.6e-7 / 4.4e-7, h14 (32 layers) 6.3e-7 / 6.5e-7.  The second call pins "224 in ->
    identity resize, no blur"."""
    from oracle import clip_ref as CR
    g, p, sd = towers(name)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    with torch.no_grad():
        e1 = rel_l2(CR.encode_image(sd, pixel_values(g["x"]).float(), p.heads, p.patch_size), g["embeds"])
        e2 = rel_l2(CR.clip_conditioner(sd, g["x"].float(), p.heads, p.patch_size, p.image_size), g["embeds"])
    print(f"\n{name}: restatement fp32 vs transformers fp64: encode_image {e1:.3e}, clip_conditioner {e2:.3e}")
    assert e1 < BOUND and e2 < BOUND


def _swap_kv(sd, block=1):
    sd = dict(sd)
    for n in ("weight", "bias"):
        k = f"visual.transformer.resblocks.{block}.attn.in_proj_{n}"
        q, kk, v = sd[k].chunk(3, 0)
        sd[k] = torch.cat([q, v, kk], 0)
    return sd


WRONG = {  # name -> (replacements for clip_ref's torch.nn.functional, heads, state-dict edit)
    "tanh_gelu": ({"gelu": lambda y: F.gelu(y, approximate="tanh")}, 4, None),
    "quick_gelu": ({"gelu": lambda y: y * torch.sigmoid(1.702 * y)}, 4, None),
    "layernorm_eps_1e-6": ({"layer_norm": lambda t, s, w, b, eps: F.layer_norm(t, s, w, b, 1e-6)}, 4, None),
    "five_heads": ({}, 5, None),
    "kv_thirds_swapped_in_one_block": ({}, 4, _swap_kv),
}


@pytest.mark.parametrize("variant", list(WRONG))
def test_fixture_rejects_wrong_tower(towers, monkeypatch, variant):
    """The fixtures discriminate: each plausible misreading of the network, put into the restatement, lands at least
    10x above the bound of the test above (measured: tanh-GELU 1.6e-4, quick-GELU 8.2e-3, eps 1e-6 3.1e-3, 5 heads
    1.1e-1, k/v swapped 4.9e-1)."""
    from oracle import clip_ref as CR
    g, p, sd = towers("tiny")
    patch, heads, edit = WRONG[variant]
    ns = types.SimpleNamespace(**{k: getattr(F, k) for k in ("conv2d", "layer_norm", "gelu", "interpolate", "pad")})
    for k, fn in patch.items():
        setattr(ns, k, fn)
    monkeypatch.setattr(CR, "F", ns)
    with torch.no_grad():
        err = rel_l2(CR.encode_image(edit(sd) if edit else sd, pixel_values(g["x"]).float(), heads, p.patch_size),
                     g["embeds"])
    print(f"\nwrong variant {variant}: rel-L2 {err:.3e}")
    assert err >= 10 * BOUND


def test_clip_engine_host_logic_vs_transformers_fixture(towers, monkeypatch):
    """seva/_clip_engine.py on the emulated kernels (tests/fake_ops.py) against the tiny fixture: weight packing, GELU
    through the GEGLU packing, the class-token row, proj^T.  Bound: that of test_engine_host_logic.py's
    test_clip_engine_orchestration_vs_restatement (f16 operands)."""
    from seva import _clip_engine
    from seva.modules import conditioner as Cd
    monkeypatch.setattr(_clip_engine, "ops", fake_ops)
    monkeypatch.setattr(_clip_engine, "require_cuda", lambda *a: None)
    monkeypatch.setattr(_clip_engine.ClipEngine, "_resolve_device", staticmethod(lambda w: torch.device("cpu")))
    g, p, sd = towers("tiny")
    with pytest.warns(RuntimeWarning, match="RANDOM-INIT"):
        cond = Cd.CLIPConditioner(p, random_init=True)
    cond.module.load_state_dict(sd, strict=True)
    got = cond(g["x"].float())
    err = rel_l2(got, g["embeds"])
    print(f"\nCLIP engine (emulated kernels) vs transformers fixture: rel-L2 {err:.3e}")
    assert got.shape == g["embeds"].shape and err < 2e-3


def test_fixture_provenance(towers):
    """The committed tiny fixture is what transformers computes: rebuild the model and compare.  A second run of the
    generator on one machine reproduces the embeddings bit for bit (rel-L2 0.0 observed); 1e-12 allows for a BLAS that
    sums in another order (fp64 rounding through 3 layers is ~1e-15).  Skips where transformers is not installed -- the
    only test of this file that may; the fixtures themselves are the check everywhere else."""
    pytest.importorskip("transformers")
    from oracle import make_goldens_clip as M
    g, p, sd = towers("tiny")
    q, n, img_seed = M.GEOMETRIES["g11_clip_tiny"]
    assert q == p and int(g["seed"]) == M.SEED and str(g["pixel_values_rule"]) == M.RULE
    assert torch.equal(M.make_image(n, img_seed), g["x"])
    err = rel_l2(M.reference_embeds(p, sd, g["x"]), g["embeds"])
    print(f"\nrebuilt transformers model vs committed embeds: rel-L2 {err:.3e}")
    assert err <= 1e-12
