"""CPU checks of the dynamic-range audit: the torch restatement of the 72-word contract (tests/fake_range_ops.py) against an
independent derivation (torch.frexp on fp64), the report arithmetic of seva.audit, the closure of ops.AUDITED / ops.NOT_AUDITED over
seva/ops.py, the recorder on the tiny model through the engine seam of tests/test_engine_host_logic.py (kernel emulations plus
the restated range operator), the finite check, and the C-ABI additions.  No GPU work happens here."""
import inspect
import math
import os
import re
import types

import pytest
import torch

import fake_ops
import fake_range_ops as R
from conftest import ROOT, load_golden

F16, F32, U8 = torch.float16, torch.float32, torch.uint8
FMT_MAX = {F32: 3.4028234663852886e38, F16: 65504.0, U8: 448.0}


def f32_bits(v: float) -> int:
    return int(torch.tensor([v], dtype=torch.float64).to(F32).view(torch.int32)[0]) & 0xFFFFFFFF


def exact_values(x: torch.Tensor) -> torch.Tensor:
    """The elements as fp64 values (every f32, f16 and e4m3 value is exact in fp64)."""
    return (x.view(torch.float8_e4m3fn).float() if x.dtype == U8 else x).double().reshape(-1)


def derive(x: torch.Tensor) -> torch.Tensor:
    """The contract from the VALUES: e(x) = floor(log2 |x|) through torch.frexp on fp64."""
    v = exact_values(x).abs()
    w = torch.zeros(72, dtype=torch.int64)
    nan, inf, zero = torch.isnan(v), torch.isinf(v), v == 0
    fin = ~(nan | inf | zero)
    w[0], w[65], w[66] = zero.sum(), inf.sum(), nan.sum()
    _, ex = torch.frexp(v[fin])  # |v| = mant * 2^ex, mant in [0.5, 1): floor(log2 |v|) = ex - 1
    w[1:65] = torch.bincount((ex.to(torch.int64) - 1).clamp(-32, 31) + 32, minlength=64)
    w[67] = (v == FMT_MAX[x.dtype]).sum()
    w[68] = f32_bits(float(v[fin].max())) if bool(fin.any()) else 0
    w[69] = f32_bits(float(v[fin].min())) if bool(fin.any()) else 0x7F800000
    w[70] = x.numel()
    return w


def all_f16() -> torch.Tensor:
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(F16)


def all_e4m3() -> torch.Tensor:
    return torch.arange(256, dtype=torch.int32).to(U8)


def f32_edges() -> torch.Tensor:
    below = lambda v: float(torch.nextafter(torch.tensor(v, dtype=F32), torch.tensor(0.0, dtype=F32)))  # noqa: E731
    vals = torch.tensor([0.0, -0.0, 1.401298464324817e-45, 2.0 ** -33, 2.0 ** -32, below(2.0 ** -32), 65504.0, below(65520.0), 65520.0,
                         2.0 ** 31, 2.0 ** 32, 3.4028234663852886e38, -3.4028234663852886e38, math.inf, -math.inf, 1.0, -2.5], dtype=F32)
    nans = torch.tensor([0x7FC00000, 0x7F800001, 0xFFC00001 - (1 << 32), 0xFFBFFFFF - (1 << 32)],
                        dtype=torch.int64).to(torch.int32).view(F32)  # quiet and signalling, both signs
    return torch.cat([vals, nans])


CASES = {"f16": all_f16, "e4m3": all_e4m3, "f32": f32_edges}


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_matches_frexp_derivation(name):
    x = CASES[name]()
    got, want = R.tensor_range(x.view(1, -1)), derive(x)
    assert torch.equal(got, want), [(i, int(got[i]), int(want[i])) for i in range(72) if got[i] != want[i]]
    assert int(got[0] + got[1:65].sum() + got[65] + got[66]) == x.numel() and int(got[71]) == 0


def test_restatement_known_words():
    w = R.tensor_range(all_f16().view(1, -1))
    assert (int(w[0]), int(w[65]), int(w[66]), int(w[67])) == (2, 2, 2 * 1023, 2)
    assert int(w[68]) == f32_bits(65504.0) and int(w[69]) == f32_bits(2.0 ** -24)
    assert int(w[1 + 32 - 24]) == 2 and int(w[1 + 32 - 15]) == 2 * 512 and int(w[1 + 32 + 15]) == 2 * 1024
    w = R.tensor_range(all_e4m3().view(1, -1))
    assert (int(w[0]), int(w[65]), int(w[66]), int(w[67])) == (2, 0, 2, 2)
    assert int(w[68]) == f32_bits(448.0) and int(w[69]) == f32_bits(2.0 ** -9) and int(w[1 + 32 + 8]) == 2 * 7
    w = R.tensor_range(torch.full((3, 5), math.nan, dtype=F16))  # nothing finite
    assert int(w[66]) == 15 and int(w[68]) == 0 and int(w[69]) == 0x7F800000
    w = R.tensor_range(torch.tensor([[1.0, 2.0 ** -40, 2.0 ** 40, 9.9]], dtype=F32), cols=3)  # clamped ends, narrowed area
    assert int(w[1]) == 1 and int(w[64]) == 1 and int(w[33]) == 1 and int(w[70]) == 3


def test_workspace_rule():
    assert R.tensor_range_workspace_numel(1, 1) == 576 and R.tensor_range_workspace_numel(1, R.WG_ELEMS + 1) == 2 * 576
    share, wgs = R.workgroups((1 << 32) + 64)
    assert share % R.WG_ELEMS == 0 and wgs <= R.MAX_WGS and share * wgs >= (1 << 32) + 64 and share * (wgs - 1) < (1 << 32) + 64


# ------------------------------------------------------------------------------------------------ report arithmetic
def _row(seq, dtype="f16", rows=4, cols=8, hist=None, zeros=0, inf=0, nan=0, at_max=0, max_abs=1.0, min_abs=1.0, **kw):
    from seva import audit
    h = [0] * 64
    for e, n in (hist or {}).items():
        h[e + 32] = n
    meta = dict(scope="s", op="gemm", output="out_f16", buffer="qkv")
    meta.update(kw)
    return audit.Row(seq=seq, dtype=dtype, rows=rows, cols=cols, zeros=zeros, inf=inf, nan=nan, at_max=at_max, max_abs=max_abs,
                     min_abs=min_abs, hist=h, **meta)


def test_report_arithmetic(tmp_path):
    from seva import audit
    a = _row(0, hist={0: 16, -15: 8, -20: 8}, max_abs=1.5, min_abs=2.0 ** -20)
    assert a.consistent() and a.headroom_bits() == math.log2(65504.0 / 1.5) and a.headroom_bits("e4m3") == math.log2(448.0 / 1.5)
    assert a.subnormal_share("f16") == 0.5 and a.subnormal_share("e4m3") == 0.5 and a.above_share("f16") == 0.0
    b = _row(1, dtype="f32", hist={16: 4, 9: 4, 3: 24}, max_abs=70000.0, min_abs=8.0)
    assert b.headroom_bits() == math.log2(65504.0 / 70000.0) < 0  # f32 rows: "if this were cast to f16"
    assert b.headroom_bits("f32") > 100 and b.above_share() == 4 / 32 and b.above_share("e4m3") == 8 / 32
    c = _row(2, dtype="e4m3", hist={8: 30}, inf=0, nan=2, at_max=5, max_abs=448.0, min_abs=256.0)
    d = _row(3, hist={2: 31}, inf=1, max_abs=4.0, min_abs=4.0)
    z = _row(4, zeros=32, max_abs=0.0, min_abs=math.inf)
    assert z.headroom_bits() == math.inf and z.subnormal_share() == 0.0 and c.headroom_bits() == 0.0
    with pytest.raises(ValueError):
        a.subnormal_share("f32")
    rep = audit.Report([a, b, c, d, z])
    assert rep.first_nonfinite() is c and audit.Report([a, b]).first_nonfinite() is None
    assert [r.seq for r in rep.worst(3)] == [2, 3, 1] and [r.seq for r in rep.worst(2, fmt="e4m3")] == [2, 3]
    assert [r.seq for r in audit.Report([a, b, z]).worst()] == [1, 0, 4]
    assert len(rep.table().splitlines()) == 6 and "qkv" in rep.table(rep.worst(1))
    path = str(tmp_path / "rep.json")
    rep.to_json(path)
    back = audit.Report.from_json(path)
    assert back.rows == rep.rows and back.rows[4].min_abs == math.inf and back.rows[0].hist == a.hist
    audit.merge_into(path := str(tmp_path / "merged.json"), "SevaEngine", rep)
    audit.merge_into(path, "ClipEngine", audit.Report([a]))
    import json
    with open(path) as f:
        data = json.load(f)
    assert sorted(data) == ["ClipEngine", "SevaEngine"] and audit.Report.from_dict(data["SevaEngine"]).rows == rep.rows


def test_row_from_words():
    from seva import audit
    w = R.tensor_range(torch.tensor([[0.0, 1.0, -3.0, math.inf, math.nan, 65504.0]], dtype=F16))
    r = audit.Row.from_words(w.tolist(), seq=0, scope="", op="x", output="out", buffer="", dtype="f16", rows=1, cols=6)
    assert (r.zeros, r.inf, r.nan, r.at_max, r.max_abs, r.min_abs) == (1, 1, 1, 1, 65504.0, 1.0) and r.consistent()
    assert r.hist[32] == 1 and r.hist[33] == 1 and r.hist[47] == 1


# ------------------------------------------------------------------------------------------------ closure over ops.py
def test_audited_tables_cover_ops():
    from seva import ops
    calls = {n for n, f in inspect.getmembers(ops, inspect.isfunction)
             if f.__module__ == ops.__name__ and re.search(r"_lib\(\)\.seva_\w+", inspect.getsource(inspect.unwrap(f)))}
    assert len(calls) > 40
    for n in sorted(calls):
        assert (n in ops.AUDITED) + (n in ops.NOT_AUDITED) == 1, f"ops.{n} calls the library and is in neither / both audit tables"
    assert not set(ops.AUDITED) & set(ops.NOT_AUDITED)
    for n, outs in ops.AUDITED.items():
        params = inspect.signature(getattr(ops, n)).parameters
        assert outs and all(o in params for o in outs), (n, outs)
    for n, why in ops.NOT_AUDITED.items():
        assert hasattr(ops, n) and why
    for n in ("gemm", "ff_fused", "ff_fused_fp8", "conv3x3", "attention", "attention_pv8", "quantize_v_fp8", "groupnorm", "layernorm",
              "softmax_rows", "timestep_embedding_f16", "silu_f16", "add_f32", "cfg_euler", "cfg_multistep", "clip_preprocess",
              "lpips_prepare", "lpips_relu_pool"):
        assert n in ops.AUDITED
    assert "rgb_to_u8" in ops.NOT_AUDITED and "frame_metrics" in ops.NOT_AUDITED


def test_output_areas():
    from seva import ops
    t = torch.zeros(6, 40, dtype=F16)
    a = dict(a=torch.zeros(6, 64, dtype=F16), w=torch.zeros(32, 64, dtype=F16), geglu=True, split_out=True)
    assert ops._audit_views("gemm", "out_f16", t, a) == [("out_f16.hi", 0, 6, 16, 40), ("out_f16.lo", 16, 6, 16, 40)]
    assert ops._audit_views("gemm", "out_f32", t.float()[2:4], dict(a, a=a["a"][:2], geglu=False, split_out=False)) == [("out_f32", 0, 2, 32, 40)]
    assert ops._as_2d(torch.zeros(2, 3, 4, 5)) == [(0, 24, 5, 5)]
    assert ops._as_2d(torch.zeros(4, 3, 10, 10)[:, :, :, :].narrow(0, 1, 2)) == [(0, 60, 10, 10)]
    assert ops._as_2d(torch.zeros(3, 4, 8)[:, :, :6]) == [(0, 12, 6, 8)]
    assert ops._as_2d(torch.zeros(5, 3, 2, 2)[::2]) == [(0, 3, 12, 24)]       # dense images, an image pitch
    assert ops._as_2d(torch.zeros(2, 3, 8)[:, :2, :4]) == [(0, 2, 4, 8), (24, 2, 4, 8)]  # no single pitch: one piece per leading index


# ------------------------------------------------------------------------------------------------ the recorder on the tiny model
def _shapes(tag):
    g = load_golden(f"g0_keys_{tag}")
    return {str(k): tuple(int(s) for s in str(v).split(",")) for k, v in zip(g["keys"], g["shapes"])}


def _cpu_engine():
    from seva import _engine, synthetic as synth
    from seva.model import Seva, SevaParams
    sd = synth.synth_state_dict(_shapes("tiny"))
    with torch.device("meta"):
        net = Seva(SevaParams(model_channels=64))
    net.load_state_dict(sd, strict=True, assign=True)
    orig = _engine.SevaEngine.__dict__["_resolve_device"]
    _engine.SevaEngine._resolve_device = staticmethod(lambda m: torch.device("cpu"))  # the engine tests' seam
    try:
        eng = _engine.SevaEngine(net, None)
    finally:
        _engine.SevaEngine._resolve_device = orig
    return eng, sd


@pytest.fixture()
def seam(monkeypatch):
    """The kernel emulations behind the engine, each audited wrapper handing its outputs on exactly as the real one does
    (`ops.audit_outputs` with the real wrapper's signature), and the restated range operator behind `ops.tensor_range`."""
    from seva import _engine, ops
    log = types.SimpleNamespace(calls=[], records=[], ranges=0)
    ns = types.SimpleNamespace(**{k: v for k, v in vars(fake_ops).items() if not k.startswith("__")})

    def wrap(name, fn, sig):
        def call(*a, **kw):
            log.calls.append(name)
            before = len(ops._AUDIT) if ops._AUDIT is not None else 0
            r = fn(*a, **kw)
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            ops.audit_outputs(name, bound.arguments)
            given = sum(bound.arguments[o] is not None for o in ops.AUDITED[name])
            log.records.append((name, given, (len(ops._AUDIT) if ops._AUDIT is not None else 0) - before))
            return r
        return call

    for name in ops.AUDITED:
        if hasattr(fake_ops, name):
            setattr(ns, name, wrap(name, getattr(fake_ops, name), inspect.signature(getattr(ops, name))))

    def counted_range(*a, **kw):
        log.ranges += 1
        return R.tensor_range(*a, **kw)

    monkeypatch.setattr(_engine, "ops", ns)
    monkeypatch.setattr(_engine, "require_cuda", lambda *a: None)
    monkeypatch.setattr(ops, "require_cuda", lambda *a: None)
    monkeypatch.setattr(ops, "tensor_range", counted_range)
    monkeypatch.setattr(ops, "tensor_range_workspace_numel", R.tensor_range_workspace_numel)
    return log


def test_recorder_on_tiny_model(seam):
    from seva import audit, ops
    eng, sd = _cpu_engine()
    g = load_golden("g3_tiny_forward")
    args = (g["x"], g["concat"], g["t"], g["crossattn"], g["dense_vector"], int(g["T"]))
    plain = eng.forward(*args).clone()
    plain_calls = list(seam.calls)
    assert seam.ranges == 0 and ops._AUDIT is None and all(n == 0 for _, _, n in seam.records)
    seam.calls.clear()
    seam.records.clear()
    with audit.record() as rec:
        with pytest.raises(Exception, match="already active"):
            audit.record().__enter__()
        out = eng.forward(*args).clone()
    assert ops._AUDIT is None
    assert seam.calls == plain_calls and torch.equal(out, plain)           # the same launches, the same result
    assert seam.ranges == len(rec) > 0
    for name, given, made in seam.records:                                  # every audited call produced its records
        assert given >= 1 and made >= given, (name, given, made)
    rep = rec.report()
    assert len(rep.rows) == len(rec) == sum(n for _, _, n in seam.records)
    assert [r.seq for r in rep.rows] == list(range(len(rep.rows))) and all(r.consistent() for r in rep.rows)
    scopes = {r.scope for r in rep.rows}
    assert len(scopes) > 20
    for s in scopes:                                                        # every scope is a state-dict prefix
        assert s and any(k.startswith(s + ".") for k in sd), s
    assert {"time_embed", "input_blocks.0.0", "out", "input_blocks.1.1.transformer_blocks.0", "input_blocks.1.1.time_mix_blocks.0"} <= scopes
    keys = {k[0] for k in eng.arena.bufs}
    for r in rep.rows:                                                      # engine-owned outputs resolve to their arena key
        if r.op == "nhwc_to_nchw_f32":
            assert r.buffer == ""                                           # (the result tensor is the caller's)
        else:
            assert r.buffer in keys, r
    qkv = [r for r in rep.rows if r.buffer == "qkv"]
    assert qkv and all(r.op == "gemm" and r.output == "out_f16" and r.dtype == "f16" for r in qkv)
    split = [r.output for r in rep.rows if r.output.endswith((".hi", ".lo"))]  # default split classes: stem, head, skip_deep
    assert split and split.count("out_f16.hi") == split.count("out_f16.lo")
    assert rep.first_nonfinite() is None
    seam.calls.clear()
    n0 = seam.ranges
    again = eng.forward(*args)
    assert seam.ranges == n0 and seam.calls == plain_calls and torch.equal(again, plain)


def test_sliced_views_resolve(seam):
    from seva import _engine, audit, ops
    arena = _engine._Arena(torch.device("cpu"))
    buf = arena.get("x32", (8, 16), F32)
    buf.copy_(torch.arange(128.0).view(8, 16))
    own = torch.ones(4, 4)
    with audit.record() as rec:
        ops.audit_mark("a.b")
        ops.audit_outputs("add_f32", {"a": None, "b": None, "out": buf[2:5]})
        ops.audit_outputs("add_f32", {"a": None, "b": None, "out": own})
    rows = rec.report().rows
    assert [(r.buffer, r.scope, r.rows * r.cols) for r in rows] == [("x32", "a.b", 48), ("", "a.b", 16)]
    assert rows[0].max_abs == 79.0 and rows[0].min_abs == 32.0
    ops.audit_mark("ignored")  # no recorder: a no-op
    ops.audit_outputs("add_f32", {"a": None, "b": None, "out": own})
    assert seam.ranges == 2


def test_check_finite(seam, monkeypatch):
    from seva import audit
    from seva import sampling as S
    from seva._native import SevaNativeError
    x = torch.randn(2, 4, 8, 8)
    audit.check_finite(x)
    assert seam.ranges == 1
    x[1, 2, 3, 4] = math.nan
    with pytest.raises(SevaNativeError, match="SEVA_AUDIT"):
        audit.check_finite(x)
    x[1, 2, 3, 4] = -math.inf
    with pytest.raises(SevaNativeError, match="1 inf and 0 NaN"):
        audit.check_finite(x)
    assert seam.ranges == 3
    # the sampler's switch: off by default, the keyword wins over the variable
    disc = S.DDPMDiscretization()
    monkeypatch.delenv("SEVA_CHECK_FINITE", raising=False)
    assert S.EulerEDMSampler(disc, None, 2, device="cpu").check_finite is False
    assert S.EulerEDMSampler(disc, None, 2, device="cpu", check_finite=True).check_finite is True
    monkeypatch.setenv("SEVA_CHECK_FINITE", "1")
    assert S.EulerEDMSampler(disc, None, 2, device="cpu").check_finite is True
    assert S.DPMPP2MSampler(disc, None, 2, device="cpu", check_finite=False).check_finite is False


def test_env_first_call_hook(seam, monkeypatch, tmp_path):
    """SEVA_AUDIT=<path>: the first call of an engine object runs under a recorder and lands in the JSON; later calls run plain."""
    import json
    from seva import audit
    eng, _ = _cpu_engine()
    eng.use_graph = False
    g = load_golden("g3_tiny_forward")
    args = (g["x"], g["concat"], g["t"], g["crossattn"], g["dense_vector"], int(g["T"]))
    monkeypatch.delenv("SEVA_AUDIT", raising=False)
    ref = eng(*args).clone()
    assert seam.ranges == 0
    path = str(tmp_path / "audit.json")
    monkeypatch.setenv("SEVA_AUDIT", path)
    first = eng(*args).clone()
    n = seam.ranges
    assert n > 0 and torch.equal(first, ref)
    eng(*args)
    assert seam.ranges == n
    with open(path) as f:
        data = json.load(f)
    assert list(data) == ["SevaEngine"] and len(audit.Report.from_dict(data["SevaEngine"]).rows) == n


# ------------------------------------------------------------------------------------------------ C-ABI additions
def test_abi_and_symbols():  # (symbols, struct and ABI version against the binding: tests/test_abi_cpu.py)
    hdr = open(os.path.join(ROOT, "include", "seva_hip.h")).read()
    assert "int seva_tensor_range(const seva_range_desc* d, seva_stream_t stream);" in hdr and "#define SEVA_RANGE_WORDS 72" in hdr
    assert f"#define SEVA_RANGE_WG_ELEMS {R.WG_ELEMS}" in hdr
    mk = open(os.path.join(ROOT, "stable-virtual-camera_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS := .*\brange\.hip\b", mk, re.M) and "FLAGS_range := -fno-vectorize -fno-slp-vectorize" in mk


# ------------------------------------------------------------------------------------------------ logical areas, buffer names, the report file
def test_logical_areas_leave_out_pad_columns():
    from seva import ops
    out = torch.zeros(2, 5, 64, dtype=F16)
    a = dict(x1=torch.zeros(2, 4, 5, 1), x2=torch.zeros(2, 7, 5, 1), split=False)
    assert ops._audit_views("nchw_to_nhwc_f16", "out_f16", out, a) == [("out_f16", 0, 10, 11, 64)]
    assert ops._audit_views("nchw_to_nhwc_f16", "out_f16", out, dict(a, split=True)) == [("out_f16.hi", 0, 10, 11, 64), ("out_f16.lo", 11, 10, 11, 64)]
    assert ops._audit_views("softmax_rows", "out_f16", torch.zeros(36, 64, dtype=F16), dict(cols=36)) == [("out_f16", 0, 36, 36, 64)]
    assert ops._audit_views("layernorm", "out_f16", torch.zeros(6, 384, dtype=U8), dict(x=torch.zeros(6, 320))) == [("out_f16", 0, 6, 320, 384)]
    assert ops._audit_views("groupnorm", "out_f8", torch.zeros(2, 9, 128, dtype=U8),
                            dict(x1=torch.zeros(2, 9, 64), x2=torch.zeros(2, 9, 32), split_out=False, split_raw=False)) == [("out_f8", 0, 18, 96, 128)]
    assert ops._audit_views("clip_preprocess", "patches_f16", torch.zeros(8, 640, dtype=F16), dict(patch=14)) == [("patches_f16", 0, 8, 588, 640)]


def test_buffers_resolve_when_recorded_not_when_reported(seam):
    """The arena key is taken at the launch: what the engines allocate (or drop) before report() cannot change it."""
    from seva import _engine, audit, ops
    arena = _engine._Arena(torch.device("cpu"))
    buf = arena.get("early", (4, 8), F32)
    buf.fill_(2.0)
    with audit.record() as rec:
        ops.audit_outputs("add_f32", {"a": None, "b": None, "out": buf})
        arena.bufs.clear()
        arena.get("late", (4, 8), F32)
    assert [r.buffer for r in rec.report().rows] == ["early"]


def test_merge_refuses_an_unusable_file(tmp_path):
    from seva import audit
    from seva._native import SevaNativeError
    rep = audit.Report([_row(0, hist={0: 32})])
    for text in ("{ not json", "[1, 2]"):
        path = tmp_path / "audit.json"
        path.write_text(text)
        with pytest.raises(SevaNativeError, match="nothing was overwritten"):
            audit.merge_into(str(path), "SevaEngine", rep)
        assert path.read_text() == text


def test_env_hook_refuses_before_the_engine_runs(seam, monkeypatch, tmp_path):
    from seva._native import SevaNativeError
    eng, _ = _cpu_engine()
    eng.use_graph = False
    g = load_golden("g3_tiny_forward")
    path = tmp_path / "audit.json"
    path.write_text("garbage")
    monkeypatch.setenv("SEVA_AUDIT", str(path))
    with pytest.raises(SevaNativeError, match="nothing was overwritten"):
        eng(g["x"], g["concat"], g["t"], g["crossattn"], g["dense_vector"], int(g["T"]))
    assert seam.calls == [] and path.read_text() == "garbage"

