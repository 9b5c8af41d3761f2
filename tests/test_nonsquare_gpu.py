"""The 1.3B network at NON-SQUARE latents and at T = 25, HIP path vs the reference.

Every other full-width network test runs a square latent (32x32, 72x72).  The engine and the dispatch planner decide from the
per-sample image size -- GroupNorm from producer statistics (hw % 64 == 0), small-image split-K (hw <= 128), window-conv tiling
(image width), the attention kernel and its K/V split (tokens per frame) -- and a square 576 x 576 frame pins each to one branch:

  pixels (W x H)   latent h x w   tokens per frame per level    widths
  576 x 576        72 x 72        5184, 1296, 324, 81           72, 36, 18, 9
  768 x 576        72 x 96        6912, 1728, 432, 108          96, 48, 24, 12
  576 x 768        96 x 72        6912, 1728, 432, 108          72, 36, 18, 9
  1024 x 576       72 x 128       9216, 2304, 576, 144          128, 64, 32, 16

a. Goldens `tests/golden/g13_*.npz`: OUTPUTS of the reference itself (CPU fp32, 1.3B synthetic weights) from
   oracle/make_goldens_nonsquare.py; inputs regenerate here from the same `seva.synthetic` seeds.  An output is stored in parts of
   whole latents (rows `idx` of the [uncond; cond] batch): all 16 at T = 8; the 25 conditional and the unconditional 0, 12, 24 at
   T = 25.  Tolerance: NET_TOL (BASELINE.json north_star) overall and per stored latent.
b. The same latent sizes at tiny width against oracle/seva_ref.py layer by layer, default engine and SEVA_GN_FUSED_STATS=2
   (producer statistics wherever hw % 64 == 0): what makes a failure of (a) locatable.
c. Bitwise promises of the README on a non-square latent at full width.
d. Census of the GEMM / conv plan rows and attention kernels each resolution launches; every row has an exact case in kernel_cases.py.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import load_golden, rel_l2
from test_model_gpu import LAYER_TOL, NET_TOL, _build, _layer_table

# name -> (T, h, w, seed): oracle/make_goldens_nonsquare.py CASES
G13 = {
    "g13_T8_72x96": (8, 72, 96, 810),
    "g13_T8_96x72": (8, 96, 72, 820),
    "g13_T8_72x128": (8, 72, 128, 830),
    "g13_T25_72x72": (25, 72, 72, 840),
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from seva import _native
    _native.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def full(dev):
    return _build("full", dev)


def _rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _wrapper_inputs(T, h, w, seed):
    """Same recipe as oracle/make_goldens_nonsquare.py:nonsquare_inputs (x, t, cond [uncond; cond])."""
    from seva import synthetic as synth
    sc = synth.synth_scene(T, (h, w), (0,), seed=seed)
    x = _rnd(2 * T, 4, h, w, seed=seed + 1)
    c = {k: torch.cat((sc["uc"][k], sc["cond"][k]), 0) for k in ("crossattn", "concat", "dense_vector")}
    t = torch.full((2 * T,), 979, dtype=torch.int64)
    return x, t, c


def _engine_inputs(dev, T, h, w, seed):
    """(x, concat, t, y, dense) on the device, as SevaEngine.forward takes them"""
    x, t, c = _wrapper_inputs(T, h, w, seed)
    return [v.to(dev) for v in (x, c["concat"], t, c["crossattn"], c["dense_vector"])]


def _load_parts(name):
    """the parts `<name>_forward_<k>.npz` of one reference output -> (rows of the [uncond; cond] batch, their latents, first part)"""
    first = load_golden(f"{name}_forward_0")
    parts = [first] + [load_golden(f"{name}_forward_{k}") for k in range(1, int(first["parts"]))]
    assert [int(p["part"]) for p in parts] == list(range(len(parts)))
    return torch.cat([p["idx"].long() for p in parts]), torch.cat([p["y"] for p in parts]), first


# ------------------------------------------------------------------------------------------------------------ a. full width vs reference
@pytest.mark.parametrize("name", list(G13))
def test_forward_vs_reference_nonsquare(dev, full, name):
    """One SGMWrapper call at 72x96, 96x72, 72x128 (T = 8, CFG batch 16) and at T = 25 (72x72, CFG batch 50: an odd half)."""
    from seva.model import SGMWrapper
    T, h, w, seed = G13[name]
    idx, ref, g = _load_parts(name)
    assert (int(g["T"]), int(g["h"]), int(g["w"]), int(g["seed"])) == (T, h, w, seed)
    assert idx.tolist() == (list(range(16)) if T == 8 else [0, 12, 24] + list(range(25, 50)))
    net, _ = full
    x, t, c = _wrapper_inputs(T, h, w, seed)
    y = SGMWrapper(net)(x.to(dev), t.to(dev), {k: v.to(dev) for k, v in c.items()}, num_frames=T).cpu()
    assert y.shape == (2 * T, 4, h, w) and torch.isfinite(y).all()
    got = y[idx]
    err = rel_l2(got, ref)
    per = [rel_l2(got[i], ref[i]) for i in range(len(idx))]
    print(f"\n1.3B forward T={T} {h}x{w} (B={2 * T}) vs REFERENCE on {len(idx)} latents: rel-L2 {err:.3e}; per latent max {max(per):.3e} "
          f"(row {int(idx[per.index(max(per))])}) min {min(per):.3e}; max-abs {float((got - ref).abs().max()):.3e} "
          f"(|ref| max {float(ref.abs().max()):.2f})")
    assert err < NET_TOL and max(per) < NET_TOL


# ------------------------------------------------------------------------------------------------------------ b. tiny width, layer-wise
TINY_SHAPES = [(2, 72, 96), (2, 96, 72), (2, 72, 128), (2, 72, 80), (25, 8, 8)]
_oracle_cache = {}


def _tiny_oracle(sd, T, h, w):
    """inputs + the oracle's output and layer trace, computed once per shape and shared by both engine settings"""
    key = (T, h, w)
    if key not in _oracle_cache:
        from oracle import seva_ref as O
        x, t, c = _wrapper_inputs(T, h, w, seed=900 + T + h + 2 * w)
        trace = {}
        torch.set_num_threads(min(16, torch.get_num_threads()))
        ref = O.sgm_wrapper_forward(sd, x, t, c, T, trace=trace)
        _oracle_cache[key] = (x, t, c, ref, trace)
    return _oracle_cache[key]


@pytest.mark.parametrize("stats", ["default", "2"], ids=["gn_stats_default", "gn_stats_2"])
@pytest.mark.parametrize("T,h,w", TINY_SHAPES, ids=[f"T{T}_{h}x{w}" for T, h, w in TINY_SHAPES])
def test_tiny_layers_on_nonsquare_latents(dev, T, h, w, stats, monkeypatch):
    """The tiny network (model_channels = 64) on the real latent sizes, every layer against the CPU oracle.  72x80 has a width that
    is a multiple of 16 and not of 32; (25, 8, 8) runs the temporal attention with 25 tokens and the joint attention over 25 frames.
    SEVA_GN_FUSED_STATS=2 makes every GroupNorm whose input has hw % 64 == 0 and C >= 128 read its producer's statistics."""
    from seva.model import SGMWrapper
    if stats == "2":
        monkeypatch.setenv("SEVA_GN_FUSED_STATS", "2")
    else:
        monkeypatch.delenv("SEVA_GN_FUSED_STATS", raising=False)
    net, sd = _build("tiny", dev)  # a fresh engine: its arena holds this shape's buffers only (what _layer_table reads)
    eng = net.engine()
    assert eng.gn_fused_stats == (2 if stats == "2" else 1)
    x, t, c, ref, trace = _tiny_oracle(sd, T, h, w)
    y = SGMWrapper(net)(x.to(dev), t.to(dev), {k: v.to(dev) for k, v in c.items()}, num_frames=T)
    torch.cuda.synchronize()
    rows = _layer_table(eng, trace, x.shape[0])
    err = rel_l2(y.cpu(), ref)
    worst = sorted(rows, key=lambda r: -r[1])[:3]
    print(f"\ntiny T={T} {h}x{w} stats={stats}: output rel-L2 {err:.3e}; {len(rows)} layers, worst "
          + ", ".join(f"{p} {e:.3e}" for p, e, _ in worst))
    assert len(rows) >= 40
    bad = [(p, e) for p, e, _ in rows if not e < LAYER_TOL]
    assert not bad, f"layers beyond tolerance: {bad[:5]}"
    assert err < NET_TOL


# ------------------------------------------------------------------------------------------------------------ c. bitwise promises
def test_forward_is_bit_repeatable_and_cfg_halves_are_independent_at_72x96(dev, full):
    """T = 8, 72x96: two eager forwards give equal bits, the hipGraph replay equals them, and the conditional half launched alone
    (batch T) is bitwise the conditional half of the CFG batch (2T) -- what the CFG split over two ranks relies on."""
    net, _ = full
    eng = net.engine()
    T = 8
    x, concat, t, y, dense = _engine_inputs(dev, T, 72, 96, 31)
    a = eng.forward(x, concat, t, y, dense, T).clone()
    b = eng.forward(x, concat, t, y, dense, T).clone()
    assert torch.isfinite(a).all() and 1e-3 < float(a.abs().mean()) < 1e2
    assert torch.equal(a, b)
    assert torch.equal(a, eng.forward_graphed(x, concat, t, y, dense, T))
    hi = eng.forward(x[T:], concat[T:], t[T:], y[T:], dense[T:], T).clone()
    lo = eng.forward(x[:T], concat[:T], t[:T], y[:T], dense[:T], T).clone()
    assert torch.equal(hi, a[T:]), "conditional half alone differs from the conditional half of the CFG batch"
    assert torch.equal(lo, a[:T])


def test_a_shape_change_leaves_nothing_behind(dev, full):
    """72x72, then 72x96, then 72x72 again on ONE engine: the third result is the first, bit for bit (no stale arena buffer, split-K
    workspace or statistics hand-off survives a change of shape)."""
    net, _ = full
    eng = net.engine()
    T = 8
    sq = _engine_inputs(dev, T, 72, 72, 41)
    ns = _engine_inputs(dev, T, 72, 96, 42)
    first = eng.forward(*sq, T).clone()
    mid = eng.forward(*ns, T).clone()
    again = eng.forward(*sq, T).clone()
    assert torch.isfinite(first).all() and torch.isfinite(mid).all()
    assert torch.equal(again, first)
    assert torch.equal(eng.forward(*ns, T), mid)


def test_whole_step_graph_is_bit_identical_to_eager_at_72x128(dev, full, monkeypatch):
    """The recipe of test_model_gpu.py::test_whole_step_graph_is_bit_identical_to_eager at full width, T = 8, 72x128: step 0 eager,
    step 1 captures the whole Euler step into one hipGraph, step 2 replays it; equal to the all-eager loop bit for bit."""
    from seva import sampling as S
    from seva import synthetic as synth
    from seva.model import SGMWrapper
    net, _ = full
    T, h, w, steps = 8, 72, 128, 3
    g = torch.Generator().manual_seed(5)
    eps = [torch.randn(T, 4, h, w, generator=g) for _ in range(steps)]
    sc = synth.synth_scene(T, (h, w), (0,), seed=23)
    disc = S.DDPMDiscretization()
    den = S.DiscreteDenoiser(disc, num_idx=1000, device=dev)
    wrap = SGMWrapper(net)

    def loop():
        sampler = S.EulerEDMSampler(disc, S.MultiviewCFG(1.2), num_steps=steps, verbose=False, device=dev, s_churn=0.0)
        it = iter(eps)
        sampler.noise_fn = lambda x: next(it).to(x.device)
        cond = {k: v.to(dev) for k, v in sc["cond"].items()}
        uc = {k: v.to(dev) for k, v in sc["uc"].items()}
        out = sampler(lambda x, s, c: den(wrap, x, s, c, num_frames=T), sc["noise"].to(dev), scale=2.0, cond=cond, uc=uc,
                      verbose=False, c2w=sc["c2w"].to(dev), K=sc["K"].to(dev), input_frame_mask=sc["input_frame_mask"].to(dev))
        return out.clone(), sampler

    eng = net.engine()
    monkeypatch.setenv("SEVA_STEPGRAPH", "0")
    monkeypatch.setenv("SEVA_HIPGRAPH", "0")
    keep = eng.use_graph
    eng.use_graph = False
    try:
        ref, s0 = loop()
    finally:
        eng.use_graph = keep
    assert s0._step_graphs.captures == 0
    monkeypatch.setenv("SEVA_STEPGRAPH", "1")
    monkeypatch.setenv("SEVA_HIPGRAPH", "1")
    got, s1 = loop()
    assert s1._step_graphs.captures == 1 and s1._step_graphs.graph.replays == steps - 1
    assert torch.isfinite(ref).all() and torch.equal(got, ref)


# ------------------------------------------------------------------------------------------------------------ d. census
def _attention_kernel(lq, lk, pre, ws, pv8=False):
    """The kernel a launch takes, as seva_attention_f16 / seva_attention_pv8 dispatch it (csrc/attention.hip, attention_fp8.hip;
    default knobs): from the launch's own arguments, so the census needs no kernel trace."""
    from seva import ops
    if pv8:
        return "pv8_kernel<true> + combine" if lk >= ops.ATTN_SPLIT_MIN_LK and ws else "pv8_kernel<false>"
    if lq <= 32:
        return "attn_kernel<1,32>"
    if pre and lq >= ops.PV8_MIN_LQ:
        return "attn16_kernel<64,true> + combine" if lk >= ops.ATTN_SPLIT_MIN_LK and ws else "attn16_kernel<64>"
    return "attn_kernel<4,64>"


CENSUS = [(8, 72, 72), (8, 72, 96), (8, 96, 72), (8, 72, 128), (25, 72, 72)]


def test_census_of_plan_rows_and_attention_kernels(dev, full, monkeypatch):
    """One eager forward per resolution with ops.gemm / conv3x3 / conv3x3_up_phases / attention / attention_pv8 wrapped:
    `ops.last_plan()` after every GEMM / conv launch, the dispatch of every attention launch.  Printed: what each resolution reaches
    that 72x72 at T = 8 does not.  Asserted: every GEMM / conv row the network really launches has an exact case in kernel_cases.py
    (the closure rule of test_kernel_coverage_cpu.py applied to the network's own launches)."""
    from kernel_cases import CASES
    from seva import ops
    net, _ = full
    eng = net.engine()
    seen = {}
    cur = {}

    def wrap_plan(name):
        fn = getattr(ops, name)

        def inner(*a, **k):
            r = fn(*a, **k)
            cur["rows"].add(ops.last_plan())
            if name == "conv3x3":  # which row each level's conv takes: image size, channels, statistics, split-K workspace
                n, ih, iw, cin = a[0].shape
                cur["convs"].add(f"{ops.last_plan()} @ {ih}x{iw} {cin}->{a[1].shape[0]}" + (" stride 2" if k.get("stride", 1) == 2 else "")
                                 + (" upsample" if k.get("upsample") else "") + (" stats" if k.get("ch_stats") is not None else "")
                                 + (" a2" if k.get("a2") is not None else "") + (" sk_ws" if k.get("splitk_ws") is not None else ""))
            return r
        monkeypatch.setattr(ops, name, inner)

    def wrap_attn(name, pv8):
        fn = getattr(ops, name)

        def inner(*a, **k):
            lq, lk, nb = k["lq"], k["lk"], k["nb0"] * k["nb1"] * k["heads"]
            kern = _attention_kernel(lq, lk, k.get("q_prescaled", False), k.get("split_ws") is not None, pv8)
            blocks = nb * ((lq + 255) // 256) if "attn16" in kern or "pv8" in kern else nb
            cur["attn"].add(f"{kern} lq={lq} lk={lk} heads={k['heads']} grid&7={blocks & 7}")
            return fn(*a, **k)
        monkeypatch.setattr(ops, name, inner)

    for name in ("gemm", "conv3x3", "conv3x3_up_phases"):
        wrap_plan(name)
    wrap_attn("attention", False)
    wrap_attn("attention_pv8", True)
    for T, h, w in CENSUS:
        cur = {"rows": set(), "attn": set(), "convs": set()}
        out = eng.forward(*_engine_inputs(dev, T, h, w, 51), T)
        assert torch.isfinite(out).all()
        seen[(T, h, w)] = cur
    base = seen[CENSUS[0]]
    print(f"\n[census] T=8 72x72: {len(base['rows'])} GEMM / conv plan rows, {len(base['attn'])} attention launches")
    for r in sorted(base["rows"]):
        print(f"[census]   row   {r}")
    for r in sorted(base["convs"]):
        print(f"[census]   conv  {r}")
    for r in sorted(base["attn"]):
        print(f"[census]   attn  {r}")
    for key in CENSUS[1:]:
        T, h, w = key
        new_rows, new_attn = seen[key]["rows"] - base["rows"], seen[key]["attn"] - base["attn"]
        print(f"[census] T={T} {h}x{w}: {len(seen[key]['rows'])} rows ({len(new_rows)} not reached at 72x72), "
              f"{len(seen[key]['attn'])} attention launches ({len(new_attn)} not reached at 72x72)")
        for r in sorted(new_rows):
            print(f"[census]   + row   {r}")
        for r in sorted(seen[key]["convs"] - base["convs"]):
            print(f"[census]   + conv  {r}")
        for r in sorted(new_attn):
            print(f"[census]   + attn  {r}")
    known = {c.row for c in CASES}
    launched = set().union(*(s["rows"] for s in seen.values()))
    assert launched and "" not in launched
    assert launched <= known, f"plan rows without an exact case in tests/kernel_cases.py: {sorted(launched - known)}"
