"""seva_tensor_range and the audit recorder on the device.  Every comparison of the kernel is torch.equal against the integer
restatement of its contract (tests/fake_range_ops.py, itself held against a frexp derivation in tests/test_range_cpu.py): counts are
integers, there is no tolerance."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import fake_range_ops as R
from conftest import load_golden
from test_range_cpu import all_e4m3, all_f16, f32_edges

F16, F32, U8 = torch.float16, torch.float32, torch.uint8
GUARD = 4096  # bytes around every buffer


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from seva import _native
    _native.load()
    return torch.device("cuda:0")


def nan_filled(numel, dtype, dev):
    if dtype == U8:
        return torch.full((numel,), 0x7F, dtype=U8, device=dev)
    return torch.full((numel,), math.nan, dtype=dtype, device=dev)


def place(data: torch.Tensor, rows: int, cols: int, pitch: int, dev, lead: int = 0) -> tuple:
    """rows x cols view at `pitch` holding `data`, inside a buffer whose every other element (pitch gap, `lead` + guard
    elements before, guard after) is a NaN: a kernel that reads outside the area counts NaNs it must not see."""
    g = GUARD // data.element_size()
    buf = nan_filled(g + lead + rows * pitch + g, data.dtype, dev)
    view = buf[g + lead: g + lead + rows * pitch].view(rows, pitch)[:, :cols]
    view.copy_(data.to(dev).reshape(rows, cols))
    return buf, view


def run(view: torch.Tensor, **kw) -> torch.Tensor:
    """ops.tensor_range with sentinels around `out` and behind the workspace's stated size; checks that both survive."""
    from seva import ops
    dev = view.device
    rows = kw.get("rows", view.shape[0] if view.dim() == 2 else 1)
    cols = kw.get("cols", view.shape[-1])
    need = ops.tensor_range_workspace_numel(rows, cols)
    assert need == R.tensor_range_workspace_numel(rows, cols)
    ws = torch.full((need + GUARD,), 0xA5, dtype=U8, device=dev)
    outb = torch.full((16 + 72 + 16,), -0x0123456789ABCDEF, dtype=torch.int64, device=dev)
    got = ops.tensor_range(view, outb[16:88], workspace=ws[:need], **kw)
    assert got.data_ptr() == outb[16:88].data_ptr()
    assert bool((ws[need:] == 0xA5).all()), "workspace written beyond seva_tensor_range_size"
    assert bool((outb[:16] == -0x0123456789ABCDEF).all()) and bool((outb[88:] == -0x0123456789ABCDEF).all()), "out guard written"
    return got.clone()


def check(view: torch.Tensor, **kw):
    got, want = run(view, **kw), R.tensor_range(view, **kw)
    assert torch.equal(got, want), [(i, int(got[i]), int(want[i])) for i in range(72) if got[i] != want[i]]
    assert int(got[0] + got[1:65].sum() + got[65] + got[66]) == int(got[70])
    return got


def tiled(x: torch.Tensor, n: int) -> torch.Tensor:
    return x.repeat(-(-n // x.numel()))[:n]


SETS = {"f16": all_f16, "e4m3": all_e4m3, "f32": f32_edges}


@pytest.mark.parametrize("name", list(SETS))
def test_exhaustive_sets_one_row(dev, name):
    x = SETS[name]()
    buf, view = place(x, 1, x.numel(), x.numel(), dev)
    got = check(view)
    assert int(got[70]) == x.numel()
    if name == "f16":
        assert (int(got[0]), int(got[65]), int(got[66]), int(got[67])) == (2, 2, 2046, 2)
    if name == "e4m3":
        assert (int(got[0]), int(got[65]), int(got[66]), int(got[67])) == (2, 0, 2, 2)


@pytest.mark.parametrize("name", list(SETS))
def test_exhaustive_sets_pitched(dev, name):
    """256 x 256 in a pitch-264 buffer (rows a whole number of 16-byte vectors apart: the vector path with a row pitch), NaN in the
    pitch gap and around the buffer."""
    x = tiled(SETS[name](), 65536)
    buf, view = place(x, 256, 256, 264, dev)
    before = buf.clone()
    check(view)
    assert torch.equal(buf.view(torch.uint8), before.view(torch.uint8)), "the input was written"


@pytest.mark.parametrize("dtype", [F16, F32, U8], ids=["f16", "f32", "e4m3"])
@pytest.mark.parametrize("rows,cols,pitch", [(1, 1, 1), (1, 7, 7), (5, 1, 9), (3, 129, 136), (7, 64, 64), (2, 48, 80)])
def test_small_shapes(dev, dtype, rows, cols, pitch):
    g = torch.Generator().manual_seed(rows * 1000 + cols)
    if dtype == U8:
        x = torch.randint(0, 256, (rows * cols,), generator=g, dtype=torch.int32).to(U8)
    else:
        x = (torch.randn(rows * cols, generator=g) * 300).to(dtype)
        x[::3] = 0.0
    buf, view = place(x, rows, cols, pitch, dev)
    check(view)


def test_base_aligned_to_two_bytes_only(dev):
    """An f16 view one element into an aligned buffer: no 16-byte loads, the element path."""
    x = all_f16()[:40001]
    buf, view = place(x, 1, x.numel(), x.numel(), dev, lead=1)
    assert view.data_ptr() % 16 == 2
    check(view)
    buf, view = place(tiled(all_f16(), 33 * 40), 33, 40, 48, dev, lead=3)  # rows a multiple of 8 apart, base odd
    assert view.data_ptr() % 16 == 6
    check(view)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_one_workgroup_share(dev, delta):
    """rows * cols at one workgroup's share (SEVA_RANGE_WG_ELEMS) and one element to either side."""
    from seva import ops
    n = ops.RANGE_WG_ELEMS + delta
    assert ops.RANGE_WG_ELEMS == R.WG_ELEMS
    assert ops.tensor_range_workspace_numel(1, n) == (2 if delta > 0 else 1) * 72 * 8
    g = torch.Generator().manual_seed(5 + delta)
    bits = torch.randint(0, 65536, (n,), generator=g, dtype=torch.int32).to(torch.int16).view(F16)
    buf, view = place(bits, 1, n, n, dev)
    check(view)
    buf, view = place(bits.view(torch.uint8)[:n].clone(), 1, n, n, dev)
    check(view)


def test_many_workgroups_odd_sizes(dev):
    g = torch.Generator(device=dev).manual_seed(11)
    x = (torch.randn((1031, 4099), generator=g, device=dev) * torch.exp2(torch.randint(-30, 18, (1031, 1), generator=g, device=dev).float())).to(F16)
    got = check(x)
    assert int(got[70]) == 1031 * 4099 and int(got[65]) > 0 and int(got[0]) > 0  # the scales reach both ends of f16
    check(x, rows=1000, cols=4000)          # a corner of it: pitch 4099, two-byte-aligned rows
    check(x.float()[:, :4096])              # f32, pitch 4099, rows of whole vectors but odd pitch: the element path


def test_four_gib_of_e4m3(dev):
    """2^32 + 64 bytes: the smallest size at which a 32-bit element index or a 32-bit count goes wrong.  Expected words in closed form."""
    n = (1 << 32) + 64
    x = torch.full((n,), 0x3C, dtype=U8, device=dev)  # 1.5
    x[n - 1] = 0xFE                                   # -448, the last element
    x[(1 << 32) + 3] = 0x80                           # -0
    x[(1 << 32) - 1] = 0x01                           # 2^-9
    got = run(x.view(1, n))
    want = torch.zeros(72, dtype=torch.int64)
    want[0], want[1 + 32 + 0], want[1 + 32 + 8], want[1 + 32 - 9], want[67], want[70] = 1, n - 3, 1, 1, 1, n
    want[68] = int(torch.tensor([448.0]).view(torch.int32)[0])
    want[69] = int(torch.tensor([2.0 ** -9]).view(torch.int32)[0])
    assert torch.equal(got.cpu(), want), [(i, int(got[i]), int(want[i])) for i in range(72) if got[i] != want[i]]


def test_rejects_bad_arguments(dev):
    from seva import ops
    from seva._native import SevaNativeError
    x = torch.zeros((4, 8), dtype=F16, device=dev)
    with pytest.raises(SevaNativeError):
        ops.tensor_range(x.double())
    with pytest.raises(SevaNativeError):
        ops.tensor_range(x.t())
    with pytest.raises(SevaNativeError):
        ops.tensor_range(x, cols=9)
    with pytest.raises(AssertionError):
        ops.tensor_range(x, workspace=torch.empty(8, dtype=U8, device=dev))


# ------------------------------------------------------------------------------------------------ the recorder on the real kernels
def _shapes(tag):
    g = load_golden(f"g0_keys_{tag}")
    return {str(k): tuple(int(s) for s in str(v).split(",")) for k, v in zip(g["keys"], g["shapes"])}


PLANT = "input_blocks.1.1.transformer_blocks.0.attn1.to_q.weight"


def _build(dev, plant=False, precision=None):
    from seva import synthetic as synth
    from seva.model import Seva, SevaParams
    sd = synth.synth_state_dict(_shapes("tiny"), 0)
    if plant:
        sd[PLANT] = sd[PLANT] * 1e6
    with torch.device("meta"):
        net = Seva(SevaParams(model_channels=64))
    net.load_state_dict(sd, strict=True, assign=True)
    net = net.to(dev).eval()
    if precision:
        net.set_precision(precision)
    return net


@pytest.fixture(scope="module")
def tiny(dev):
    return _build(dev)


@pytest.fixture(scope="module")
def planted(dev):
    return _build(dev, plant=True)


def _forward(net, dev):
    from seva.model import SGMWrapper
    g = load_golden("g3_tiny_forward")
    c = {k: g[k].to(dev) for k in ("crossattn", "concat", "dense_vector")}
    with torch.no_grad():
        return SGMWrapper(net)(g["x"].to(dev), g["t"].to(dev), c, num_frames=int(g["T"])).clone()


def test_tiny_model_bit_equal_and_consistent(dev, tiny):
    from seva import audit, ops
    plain = _forward(tiny, dev)
    with audit.record() as rec:
        out = _forward(tiny, dev)
    assert ops._AUDIT is None and torch.equal(out, plain)
    after = _forward(tiny, dev)
    assert torch.equal(after, plain)
    rep = rec.report()
    assert len(rep.rows) > 100 and all(r.consistent() for r in rep.rows)
    assert rep.first_nonfinite() is None
    keys = {k[0] for k in tiny.engine().arena.bufs}
    assert all(r.buffer in keys for r in rep.rows if r.op != "nhwc_to_nchw_f32")
    worst = rep.worst(5)
    assert worst[0].headroom_bits() <= worst[-1].headroom_bits() and rep.table(worst).count("\n") == 5


def test_planted_overflow_is_named(dev, planted):
    from seva import audit
    with audit.record() as rec:
        _forward(planted, dev)
    rep = rec.report()
    bad = rep.first_nonfinite()
    assert bad is not None
    print(bad)
    assert bad.scope == "input_blocks.1.1.transformer_blocks.0" and bad.op == "gemm" and bad.buffer == "qkv"
    assert all(r.inf + r.nan == 0 for r in rep.rows if r.seq < bad.seq)
    assert all(r.consistent() for r in rep.rows)


@pytest.mark.parametrize("precision", ["f16", "fp8"])
def test_weights_report(dev, precision):
    from seva import audit
    net = _build(dev, precision=precision)
    rep = audit.weights(net)
    W = net.engine().W
    floats = {}
    for k, t in W.items():
        if t.dtype in (F32, F16, U8) and t.numel() and not k.endswith("8e"):
            floats.setdefault((t.data_ptr(), t.dtype), k)
    assert len(rep.rows) == len(floats) and all(r.consistent() and r.op == "weights" for r in rep.rows)
    by_key = {r.output: r for r in rep.rows}
    spots = ["time_embed.0.w", "out.2.w", "emb_all.b"]
    if precision == "fp8":
        spots[0] = next(k for k in W if k.endswith(".qkv8"))
        assert by_key[spots[0]].dtype == "e4m3" and 224.0 < by_key[spots[0]].max_abs <= 448.0  # every row's maximum sits in the top binade
    for k in spots:
        t = W[k]
        want = float((t.view(torch.float8_e4m3fn) if t.dtype == U8 else t).float().abs().max())
        assert by_key[k].max_abs == want, (k, by_key[k].max_abs, want)
        assert by_key[k].rows * by_key[k].cols == t.numel()


def _sample(net, dev, monkeypatch, flag):
    from seva import sampling as S
    from seva import synthetic as synth
    from seva.model import SGMWrapper
    T, hw = 3, 16
    if flag is None:
        monkeypatch.delenv("SEVA_CHECK_FINITE", raising=False)
    else:
        monkeypatch.setenv("SEVA_CHECK_FINITE", flag)
    sc = synth.synth_scene(T, (hw, hw), (0,), seed=23)
    disc = S.DDPMDiscretization()
    den = S.DiscreteDenoiser(disc, num_idx=1000, device=dev)
    sampler = S.EulerEDMSampler(disc, S.MultiviewCFG(1.2), num_steps=2, verbose=False, device=dev, s_churn=0.0)
    sampler.noise_fn = torch.zeros_like
    wrap = SGMWrapper(net)
    cond = {k: v.to(dev) for k, v in sc["cond"].items()}
    uc = {k: v.to(dev) for k, v in sc["uc"].items()}
    return sampler(lambda x, s, c: den(wrap, x, s, c, num_frames=T), sc["noise"].to(dev), scale=2.0, cond=cond, uc=uc,
                   verbose=False, c2w=sc["c2w"].to(dev), K=sc["K"].to(dev), input_frame_mask=sc["input_frame_mask"].to(dev))


def test_check_finite_switch(dev, tiny, planted, monkeypatch):
    from seva._native import SevaNativeError
    off = _sample(tiny, dev, monkeypatch, None)
    on = _sample(tiny, dev, monkeypatch, "1")
    assert torch.equal(on, off) and bool(torch.isfinite(on).all())
    with pytest.raises(SevaNativeError, match="SEVA_AUDIT"):
        _sample(planted, dev, monkeypatch, "1")
    assert not bool(torch.isfinite(_sample(planted, dev, monkeypatch, None)).all())  # off: the NaN latent comes back silently, as before


def test_check_finite_adds_one_range_call_only_when_on(dev, tiny, monkeypatch):
    from seva import ops
    calls = []
    real = ops.tensor_range
    monkeypatch.setattr(ops, "tensor_range", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    _sample(tiny, dev, monkeypatch, None)
    assert len(calls) == 0
    _sample(tiny, dev, monkeypatch, "1")
    assert len(calls) == 1


# ------------------------------------------------------------------------------------------------ a whole sampler call under a recorder
class _Run:
    """One sampler object and one set of inputs, called as often as a test likes (same cache keys every time)."""

    def __init__(self, net, dev, steps=3, solver=None):
        from seva import sampling as S
        from seva import synthetic as synth
        from seva.model import SGMWrapper
        T, hw = 3, 16
        sc = synth.synth_scene(T, (hw, hw), (0,), seed=23)
        disc = S.DDPMDiscretization()
        den = S.DiscreteDenoiser(disc, num_idx=1000, device=dev)
        self.sampler = S.EulerEDMSampler(disc, S.MultiviewCFG(1.2), num_steps=steps, verbose=False, device=dev, s_churn=0.0,
                                         solver=solver, check_finite=False)
        self.sampler.noise_fn = torch.zeros_like
        wrap = SGMWrapper(net)
        self.denoiser = lambda x, s, c: den(wrap, x, s, c, num_frames=T)
        self.noise = sc["noise"].to(dev)
        self.kw = dict(scale=2.0, cond={k: v.to(dev) for k, v in sc["cond"].items()}, uc={k: v.to(dev) for k, v in sc["uc"].items()},
                       verbose=False, c2w=sc["c2w"].to(dev), K=sc["K"].to(dev), input_frame_mask=sc["input_frame_mask"].to(dev))

    def __call__(self):
        return self.sampler(self.denoiser, self.noise.clone(), **self.kw).clone()


@pytest.mark.parametrize("solver", ["euler", "dpmpp2m"])
@pytest.mark.parametrize("warmed", [False, True], ids=["fresh", "warmed"])
def test_sampler_call_under_recorder(dev, tiny, solver, warmed, recwarn):
    """A 3-step sampler call under audit.record(): every step's launches are recorded (no whole-step capture or replay while
    the recorder is active), the result is the plain run's bit for bit, and the sampler's step graphs work afterwards."""
    from seva import audit
    ref = _Run(tiny, dev, solver=solver)()
    run = _Run(tiny, dev, solver=solver)
    cache = run.sampler._step_graphs
    if warmed:  # the step graph exists before the recorder opens
        assert torch.equal(run(), ref) and cache.captures >= 1
    before = cache.captures
    with audit.record() as rec:
        out = run()
    rep = rec.report()
    assert torch.equal(out, ref)
    assert not [w for w in recwarn.list if "capture failed" in str(w.message)]
    assert not cache.disabled and cache.captures == before              # nothing captured, nothing switched off
    step_ops = ("cfg_multistep",) if solver == "dpmpp2m" else ("cfg_euler", "euler_step")
    assert sum(r.op == "nhwc_to_nchw_f32" for r in rep.rows) == 3 and sum(r.op in step_ops and r.output == "out" for r in rep.rows) == 3
    assert sum(r.op == "denoiser_combine" for r in rep.rows) == 3 and all(r.consistent() for r in rep.rows)
    assert rep.first_nonfinite() is None
    assert torch.equal(run(), ref)                                      # plain again: replays its graph, or captures it now
    assert not cache.disabled and cache.captures == max(before, 1) and cache.graph is not None and cache.graph.replays >= 1
    assert torch.equal(run(), ref) and cache.captures == max(before, 1)  # and the next trajectory replays the same graph
    assert not [w for w in recwarn.list if "capture failed" in str(w.message)]


# ------------------------------------------------------------------------------------------------ VAE and CLIP engines
def _check_engine_report(rep, sd_keys, arena_keys, caller_ops):
    assert len(rep.rows) > 20 and all(r.consistent() for r in rep.rows) and rep.first_nonfinite() is None
    for s in {r.scope for r in rep.rows}:
        assert s and any(k.startswith(s + ".") for k in sd_keys), s
    for r in rep.rows:
        assert (r.buffer in arena_keys) or r.op in caller_ops, r


@pytest.mark.parametrize("precision", ["f16", "fp8"])
def test_vae_engines_under_recorder(dev, precision, monkeypatch, tmp_path):
    import json
    from oracle import vae_ref as V
    from seva import audit, synthetic as synth
    from seva.modules.autoencoder import AutoEncoder, VaeWeights
    monkeypatch.delenv("SEVA_AUDIT", raising=False)
    block_out = (128, 256, 512, 512)
    ae = AutoEncoder(chunk_size=1, random_init=True)
    if tuple(block_out) != tuple(ae.module.block_out):
        ae.module = VaeWeights(block_out=block_out)
    sd = synth.synth_state_dict({**V.decoder_shapes(block_out=block_out), **V.encoder_shapes(block_out=block_out)}, 3)
    ae.module.load_state_dict(sd)
    ae = ae.to(dev)
    ae.set_precision(precision, encode=precision)
    ae.set_upsample("phases")
    g = torch.Generator().manual_seed(1)
    z = (torch.randn(1, 4, 16, 16, generator=g) * 0.18215 * 4).to(dev)
    x = (torch.rand(1, 3, 128, 128, generator=g) * 2 - 1).to(dev)
    dec, enc = ae.decode(z).clone(), ae.encode(x).clone()
    with audit.record() as rec:
        dec_a = ae.decode(z).clone()
    with audit.record() as rec_e:
        enc_a = ae.encode(x).clone()
    assert torch.equal(dec_a, dec) and torch.equal(enc_a, enc)
    assert torch.equal(ae.decode(z), dec) and torch.equal(ae.encode(x), enc)
    rd, re_ = rec.report(), rec_e.report()
    _check_engine_report(rd, sd, {k[0] for k in ae.engine().arena.bufs}, ("nhwc_to_nchw_f32",))
    _check_engine_report(re_, sd, {k[0] for k in ae.encoder_engine().arena.bufs}, ("nhwc_to_nchw_f32", "scale_rows"))
    ops_seen = {r.op for r in rd.rows} | {r.op for r in re_.rows}
    assert {"softmax_rows", "groupnorm", "conv3x3", "gemm", "nchw_to_nhwc_f16"} <= ops_seen
    soft = [r for r in rd.rows if r.op == "softmax_rows"]
    assert soft and all(r.cols == 256 and r.max_abs <= 1.0 for r in soft)           # the 16 x 16 tokens, not the padded row
    lat = [r for r in rd.rows if r.op == "nchw_to_nhwc_f16"]
    assert lat and all(r.cols == 4 for r in lat)                                     # the latent's channels, not the 64-wide operand
    assert any(r.dtype == "e4m3" for r in rd.rows) == (precision == "fp8")
    # the packed weights: only the packs the engines hold
    held = {(t.data_ptr(), t.dtype) for e in (ae.engine(), ae.encoder_engine()) for n in ("W", "W8", "W4") if getattr(e, n, None)
            for k, t in getattr(e, n).items() if t.dtype in (F32, F16, U8) and t.numel() and not k.endswith("8e")}
    assert (ae.engine().W8 is not None) == (precision == "fp8") and ae.engine().W4 is not None
    rw = audit.weights(ae)
    assert (ae.engine().W8 is not None) == (precision == "fp8")                       # nothing was packed for the report
    assert len(rw.rows) == len(held) and all(r.consistent() for r in rw.rows) and {r.scope for r in rw.rows} == {"VaeDecoderEngine", "VaeEncoderEngine"}
    assert any(r.dtype == "e4m3" for r in rw.rows) == (precision == "fp8")
    # SEVA_AUDIT: the first call of a new engine object lands in the file, keyed by class
    path = tmp_path / "audit.json"
    monkeypatch.setenv("SEVA_AUDIT", str(path))
    ae._engine = ae._enc_engine = None
    assert torch.equal(ae.decode(z), dec) and torch.equal(ae.encode(x), enc) and torch.equal(ae.decode(z), dec)
    data = json.loads(path.read_text())
    assert sorted(data) == ["VaeDecoderEngine", "VaeEncoderEngine"] and len(audit.Report.from_dict(data["VaeDecoderEngine"]).rows) == len(rd.rows)


def test_clip_engine_under_recorder(dev):
    from oracle import clip_ref as CR
    from seva import audit
    from seva.modules.conditioner import CLIPConditioner, ViTParams
    p = ViTParams(width=320, layers=3, embed_dim=128)
    with pytest.warns(RuntimeWarning):
        cond = CLIPConditioner(p, random_init=True)
    sd = CR.synthetic_state_dict(p, 11)
    cond.module.load_state_dict(sd, strict=True)
    cond = cond.to(dev)
    x = (torch.rand(2, 3, 160, 200, generator=torch.Generator().manual_seed(7)) * 2 - 1).to(dev)
    ref = cond(x).clone()
    with audit.record() as rec:
        out = cond(x).clone()
    assert torch.equal(out, ref) and torch.equal(cond(x), ref)
    rep = rec.report()
    _check_engine_report(audit.Report(rep.rows[:-1]), sd, {k[0] for k in cond.engine().arena.bufs}, ())
    last = rep.rows[-1]
    assert last.op == "gemm" and last.buffer == "" and last.scope == "visual.ln_post"  # the embedding is the caller's tensor
    assert {"clip_preprocess", "attention_small", "layernorm", "gemm"} <= {r.op for r in rep.rows}
    pre = [r for r in rep.rows if r.op == "clip_preprocess"]
    assert len(pre) == 1 and pre[0].cols == 3 * p.patch_size ** 2 and pre[0].buffer == "patches"
    rw = audit.weights(cond)
    W = cond.engine().W
    assert len(rw.rows) == len({(t.data_ptr(), t.dtype) for t in W.values() if t.dtype in (F32, F16) and t.numel()})
    assert {r.output: r for r in rw.rows}["proj.w"].max_abs == float(W["proj.w"].float().abs().max())
