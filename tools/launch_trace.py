"""Launch trace of the Python host layer, on the CPU: which C-ABI calls the engines and `seva.ops` make, with which descriptors.

    python tools/launch_trace.py TREE [--out DIR] [--against DIGESTS]

imports the package and the test helpers from the checkout TREE, replaces the loaded library by a stub that records every `seva_*`
call (symbol, every descriptor field, every scalar) and returns 0, and runs the engines, the operators and the sampler (three steps
per solver and guider: on the CPU a step is not eligible for capture, so this is its eager path) on CPU tensors: nothing is computed,
so a configuration costs a second or two whatever the image size.  Pointers are canonicalised afterwards: a value inside a tensor of
`eng.W`, the arena or the inputs becomes (kind, key, byte offset), any other one the ordinal of its first appearance.  A record =
the engine's scalar attributes, a SHA-256 per packed weight, the arena's keys, the calls.  A host-side refactor must leave every
record byte-identical: run the tool on a worktree of the parent commit and on the new tree, and hand the first run's digest file
to the second through --against (exit status 1 on any difference; --out keeps the records for a diff).

The sampler's opt-in modes (`cache_interval`, `guidance_interval`, `guidance_rescale`; as arguments and through their SEVA_* variables)
run ten steps behind a network that writes its batch and the depth asked of it into the record, and the record states the options the
sampler resolved.  The drivers (`seva.pipeline.run_trajectory` / `run_views`, one process) do compute, on the torch emulation of the
operators that tests/ keeps: their record is the plan, what every window's sampler was built with, the timers' keys and a SHA-256 of
each result.

The tool fails if its configurations together never reach one of the features in the table that `coverage()` prints.
"""
import argparse
import bisect
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("tree", help="checkout to import seva, tests/ and oracle/ from")
ap.add_argument("--out", help="directory for the records (one text file per configuration) and digests.txt")
ap.add_argument("--against", help="digests.txt of another run: print both columns, fail on a difference")
args = ap.parse_args()
TREE = os.path.abspath(args.tree)
sys.path[:0] = [os.path.join(TREE, "stable-virtual-camera_amd"), os.path.join(TREE, "tests"), TREE]

import torch  # noqa: E402

from seva import _clip_engine, _engine, _native as nv, _vae_engine, ops, synthetic as synth  # noqa: E402

F16, F32, U8 = torch.float16, torch.float32, torch.uint8
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------------------------------ the stub library
class StubLib:
    """Stands in for libseva_hip.so: every symbol of `_native.SYMBOLS` records its arguments and succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name not in nv.SYMBOLS:
            raise AttributeError(name)
        return lambda *a: self._call(name, a)

    def _call(self, name, a):
        if name in ("seva_last_error", "seva_last_plan", "seva_target_arch"):
            return b""
        if name == "seva_abi_version":
            return nv.ABI_VERSION
        if name == "seva_attn_v_fp8_size":
            # include/seva_hip.h: per (sample, head) and 128-key step (keys >= lk zero-padded), 128 x 64 e4m3 values and one scale
            # byte per 32 keys and channel
            steps = a[0] * a[1] * ((a[2] + 127) // 128)
            a[3]._obj.value, a[4]._obj.value = steps * 128 * 64, steps * 4 * 64
        rec = []
        for i, (v, ty) in enumerate(zip(a, nv.SYMBOLS[name][1])):
            obj = getattr(v, "_obj", None)
            if isinstance(obj, C.Structure):
                for f, fty in obj._fields_:
                    rec.append((f, fty is C.c_void_p, getattr(obj, f)))
            elif obj is not None:
                rec.append((f"arg{i}", False, "byref"))
            else:
                if isinstance(v, C.c_void_p):
                    v = v.value
                rec.append((f"arg{i}", ty is C.c_void_p, v.decode() if isinstance(v, bytes) else v))
        self.calls.append((name, rec))
        return 0


LIB = StubLib()
nv._lib = LIB
for mod in (nv, ops):
    mod.stream_ptr = lambda device=None: 0
for mod in (nv, ops, _engine, _vae_engine, _clip_engine):
    mod.require_cuda = lambda *a: None
for cls in (_engine.SevaEngine, _vae_engine.VaeDecoderEngine, _vae_engine.VaeEncoderEngine, _clip_engine.ClipEngine):
    cls._resolve_device = staticmethod(lambda module: CPU)


def canonical(calls, spaces):
    """[(symbol, [(field, is_pointer, value)])] -> text lines; spaces: [(kind, {key: tensor})] in order of precedence."""
    ranges = []
    for kind, tensors in spaces:
        for key, t in tensors.items():
            if isinstance(t, torch.Tensor) and t.numel():
                ranges.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), kind, str(key)))
    ranges.sort(key=lambda r: r[0])
    starts = [r[0] for r in ranges]
    ordinals = {}

    def pointer(v):
        if not v:
            return 0
        i = bisect.bisect_right(starts, v) - 1
        if i >= 0 and v < ranges[i][1]:
            return [ranges[i][2], ranges[i][3], v - ranges[i][0]]
        return ["ptr", ordinals.setdefault(v, len(ordinals))]

    return [f"call {sym} " + json.dumps([[f, pointer(v) if is_ptr else v] for f, is_ptr, v in rec]) for sym, rec in calls]


def tensor_lines(kind, tensors):
    out = []
    for key, t in tensors.items():
        if isinstance(t, torch.Tensor):
            sha = hashlib.sha256(t.detach().contiguous().view(-1).view(U8).numpy().tobytes()).hexdigest()
            out.append(f"{kind} {key} {str(t.dtype)[6:]} {list(t.shape)} {sha}")
    return out


def scalar(v):
    if isinstance(v, (str, int, float, bool, type(None))):
        return True
    if isinstance(v, (set, frozenset, tuple, list)):
        return all(scalar(e) for e in v)
    return isinstance(v, dict) and all(isinstance(k, str) and scalar(e) for k, e in v.items())


def attribute_lines(eng):
    out = []
    for k, v in sorted(vars(eng).items()):
        if not k.startswith("_") and scalar(v):
            out.append(f"attr {k} = " + json.dumps(sorted(v) if isinstance(v, (set, frozenset)) else v, sort_keys=True))
    return out


@contextlib.contextmanager
def environment(env):
    saved = {k: v for k, v in os.environ.items() if k.startswith("SEVA_")}
    for k in saved:
        del os.environ[k]
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(saved)


def traced(run, spaces):
    """lines of the calls `run()` makes; `spaces()` names the tensors afterwards"""
    del LIB.calls[:]
    keep = run()  # (results stay alive until the pointers are named: a freed block could be handed out again)
    RAW.extend(LIB.calls)
    lines = canonical(LIB.calls, spaces())
    del keep
    return lines


RAW = []      # every recorded call of every configuration, for the coverage table
RECORDS = {}  # name -> text


def record(name, lines):
    assert name not in RECORDS, name
    RECORDS[name] = "\n".join(lines) + "\n"
    n_calls = sum(ln.startswith("call ") for ln in lines)
    print(f"{hashlib.sha256(RECORDS[name].encode()).hexdigest()[:20]}  {n_calls:5d} calls  {name}", flush=True)


def env_tag(env, **opts):
    parts = [f"{k[5:]}={v}" for k, v in env.items()] + [f"{k}={v}" for k, v in opts.items() if v is not None]
    return " ".join(parts) or "default"


# ------------------------------------------------------------------------------------------------------------------ UNet
_NETS = {}


def unet(tag):
    if tag not in _NETS:
        from seva.model import Seva, SevaParams
        # "phase": one level of 320 channels under the top, so that the Upsample conv takes ops.conv3x3_up_phases (c % 160 == 0)
        params = SevaParams(model_channels=64) if tag == "tiny" else SevaParams(
            model_channels=64, channel_mult=[1, 5], transformer_depth=[1, 1], attention_resolutions=[2, 1])
        with torch.device("meta"):
            net = Seva(params)
        net.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}), strict=True, assign=True)
        _NETS[tag] = net
    return _NETS[tag]


UNET_INPUTS = {"T3_8x24_lc1": (3, 8, 24, 1), "T2_8x8_lc3": (2, 8, 8, 3), "T3_96x96_lc1": (3, 96, 96, 1)}
UNET_INPUTS_SHALLOW = {**UNET_INPUTS, "T2_16x16_lc1": (2, 16, 16, 1)}  # (`unet_record`'s default is every key of UNET_INPUTS)


def unet_inputs(T, h, w, lc):
    n = 2 * T
    return {"x": torch.zeros(n, 11, h, w), "t": torch.zeros(n, dtype=torch.int64), "y": torch.zeros(n, lc, 1024),
            "dense": torch.zeros(n, 6, h, w)}, T


def unet_record(env, net="tiny", inputs=tuple(UNET_INPUTS), forward=True, **opts):
    """One engine under `env` / the constructor options, then one eager forward per input (the arena carries over)."""
    name = f"unet[{net}] {env_tag(env, **opts)}" + ("" if forward else " (attributes)")
    with environment(env):
        eng = _engine.SevaEngine(unet(net), opts.get("precision"), attention=opts.get("attention"), ff=opts.get("ff"),
                                 split=opts.get("split"))
        lines = attribute_lines(eng)
        if forward:
            lines += tensor_lines("W", eng.W)
            for key in inputs:
                inp, T = unet_inputs(*UNET_INPUTS[key])
                lines.append(f"input {key}")
                lines += traced(lambda: eng.forward(inp["x"], None, inp["t"], inp["y"], inp["dense"], T),
                                lambda: [("in", inp), ("W", eng.W), ("arena", eng.arena.bufs)])
            lines += [f"arena {k}" for k in eng.arena.bufs]
    record(name, lines)


SHALLOW_WITH_STATS = []  # (record, L) of every shallow call whose entering tensor came with its producer's statistics


def unet_shallow_record(env, key):
    """One engine under `env`: a full eager forward of input `key`, then the shallow forwards L = 1, 2, 3 of the same signature."""
    name = f"unet[tiny] {env_tag(env)} shallow {key}"
    with environment(env):
        eng = _engine.SevaEngine(unet("tiny"))
        inp, T = unet_inputs(*UNET_INPUTS_SHALLOW[key])
        lines = attribute_lines(eng)
        nout = len(eng.layout.output_blocks)
        for L in (0, 1, 2, 3):
            lines.append(f"input {key} shallow_levels={L}")
            calls = traced(lambda: eng.forward(inp["x"], None, inp["t"], inp["y"], inp["dense"], T, shallow_levels=L),
                           lambda: [("in", inp), ("W", eng.W), ("arena", eng.arena.bufs)])
            lines += calls
            if L:
                # the arena buffer that enters the first output block this call runs: the last operator of the block before it
                first = nout - (eng.shallow_input_blocks(L) + 1)
                entry = "('out:" + eng.layout.output_blocks[first - 1][-1].prefix + "'"
                reads = 0
                for ln in calls:
                    if ln.startswith("call seva_groupnorm_f16 "):
                        f = dict(json.loads(ln.split(" ", 2)[2]))
                        for x, st in (("x1", "stats1"), ("x2", "stats2")):
                            if isinstance(f[x], list) and f[x][0] == "arena" and f[x][1].startswith(entry) and f[x][2] == 0:
                                reads += 1
                                if f[st]:
                                    SHALLOW_WITH_STATS.append((name, L))
                assert reads == 1, (name, L, reads)  # exactly one GroupNorm reads the entering tensor
        lines += [f"arena {k}" for k in eng.arena.bufs]
    record(name, lines)


def unet_configurations():
    from test_engine_switches_cpu import CPU_CONFIGS
    from test_engine_switches_gpu import FULL_ENV_CONFIGS, TINY_ENV_CONFIGS, VAE_CONFIGS  # noqa: F401 (VAE_CONFIGS: vae_configurations)
    envs = [{}] + [env for env, _ in CPU_CONFIGS + TINY_ENV_CONFIGS + FULL_ENV_CONFIGS]
    envs += [{"SEVA_SPLIT_PRECISION": t} for t in ("none", "all") + tuple(_engine.SPLIT_TOKENS)]
    sliced = {"SEVA_SLICE_FRAMES": 1, "SEVA_SLICE_MIN_MB": 0}
    envs += [sliced, {**sliced, "SEVA_SLICE_ATTN": 1}, {**sliced, "SEVA_FF_FUSED": 0}, {"SEVA_UPSAMPLE_PHASES": 0}, {"SEVA_ATTN_SPLIT_KV": 0}]
    envs += [{"SEVA_ATTN_SPLIT": v} for v in (1, 3, 9)]
    for i, env in enumerate(envs):
        if env not in envs[:i]:
            unet_record(env)
    for env in ({}, {"SEVA_FP8_ATTENTION": 1}, {"SEVA_FP8_FF": 1}, {"SEVA_FP8_PAD": 1}):
        unet_record(env, precision="fp8")
    unet_record({}, precision="fp8", attention="fp8", ff="fp8")
    unet_record({}, split="all")
    for env in ({}, {"SEVA_UPSAMPLE_PHASES": 0}, {"SEVA_SPLIT_PRECISION": "resample"}, {"SEVA_FP8_PAD": 1, "SEVA_PRECISION": "fp8"}):
        unet_record(env, net="phase", inputs=("T3_8x24_lc1",))
    # parse corner values of the boolean switches: the attribute block only
    for sw in ("SEVA_FP8_ATTENTION", "SEVA_FP8_FF", "SEVA_FP8_PAD", "SEVA_FF_FUSED", "SEVA_CONV_SPLITK", "SEVA_ATTN_SPLIT_KV",
               "SEVA_FOLD_SKIP", "SEVA_HIPGRAPH", "SEVA_SLICE_ATTN"):
        for v in ("", "0", "1", "2", "yes"):
            unet_record({sw: v}, forward=False, precision="fp8" if "FP8" in sw else None)
    for v in ("", "1", "2", "yes"):  # read at every `_resample` call: needs the forward ("0": above)
        unet_record({"SEVA_UPSAMPLE_PHASES": v}, net="phase", inputs=("T2_8x8_lc3",))
    # shallow calls: where the default rule gives the entry points statistics, and a small input under the rule of the tests
    unet_shallow_record({}, "T3_96x96_lc1")
    unet_shallow_record({"SEVA_GN_FUSED_STATS": 2}, "T2_16x16_lc1")


# ------------------------------------------------------------------------------------------------------------------ VAE, CLIP
VAE_BLOCK_OUT = (64, 64, 128, 128)  # tests/test_engine_host_logic.py: same topology, narrower


def vae_weights():
    from oracle import vae_ref as V
    from seva.modules.autoencoder import VaeWeights
    wts = VaeWeights(block_out=VAE_BLOCK_OUT)
    wts.load_state_dict(synth.synth_state_dict({**V.decoder_shapes(block_out=VAE_BLOCK_OUT), **V.encoder_shapes(block_out=VAE_BLOCK_OUT)}, 5))
    return wts


def vae_record(side, env, shape, forward=True, **opts):
    name = f"vae {side} {env_tag(env, **opts)} {'x'.join(map(str, shape))}" + ("" if forward else " (attributes)")
    with environment(env):
        wts = vae_weights()
        eng = (_vae_engine.VaeDecoderEngine if side == "decode" else _vae_engine.VaeEncoderEngine)(wts, **opts)
        lines = attribute_lines(eng)
        if forward:
            lines += tensor_lines("W", eng.W)
            inp = {"x": torch.zeros(shape)}
            lines += traced(lambda: (eng.decode if side == "decode" else eng.encode)(inp["x"], 0.18215),
                            lambda: [("in", inp), ("W", eng.W), ("W8", eng.W8 or {}), ("W4", getattr(eng, "W4", None) or {}),
                                     ("arena", eng.arena.bufs)])
            lines += tensor_lines("W8", eng.W8 or {}) + tensor_lines("W4", getattr(eng, "W4", None) or {})
            lines += [f"arena {k}" for k in eng.arena.bufs]
    record(name, lines)


def vae_configurations():
    from test_engine_switches_gpu import VAE_CONFIGS
    dec, enc = (2, 4, 6, 6), (2, 3, 48, 64)
    for env in [e for e, _ in VAE_CONFIGS]:
        vae_record("decode", env, dec)
        vae_record("encode", env, enc)
    vae_record("decode", {}, dec, precision="fp8")
    vae_record("encode", {}, enc, precision="fp8")
    vae_record("decode", {"SEVA_VAE_FP8_UPSAMPLE": 1}, dec, precision="fp8")
    vae_record("encode", {"SEVA_VAE_FP8_DOWNSAMPLE": 1}, enc, precision="fp8")
    vae_record("decode", {}, (1, 4, 8, 8), upsample="phases")
    vae_record("decode", {}, dec, upsample="phases")
    vae_record("decode", {}, (1, 4, 8, 8), precision="fp8", upsample="phases")
    vae_record("decode", {"SEVA_VAE_UPSAMPLE_PHASES": 1}, (1, 4, 8, 8))
    for sw, side in (("SEVA_VAE_FOLD_SHORTCUT", "decode"), ("SEVA_VAE_UPSAMPLE_PHASES", "decode"), ("SEVA_VAE_FP8_UPSAMPLE", "decode"),
                     ("SEVA_VAE_FP8_DOWNSAMPLE", "encode"), ("SEVA_GN_FUSED_STATS", "encode")):
        for v in ("", "0", "1", "2", "yes"):
            if sw == "SEVA_GN_FUSED_STATS" and v in ("", "yes"):
                continue  # an integer switch: these two do not parse
            vae_record(side, {sw: v}, (), forward=False)
    lines = []
    for var, fn in (("SEVA_VAE_PRECISION", "vae_precision_from_env"), ("SEVA_VAE_ENCODE_PRECISION", "vae_encode_precision_from_env"),
                    ("SEVA_VAE_UPSAMPLE_PHASES", "vae_upsample_from_env"), ("SEVA_VAE_FP8_DOWNSAMPLE", "fp8_downsample_from_env"),
                    ("SEVA_VAE_FP8_UPSAMPLE", "fp8_upsample_from_env")):
        for v in (None, "", "0", "1", "2", "yes", "f16", "fp8", "bf16"):
            with environment({} if v is None else {var: v}):
                try:
                    got = getattr(_vae_engine, fn)()
                except ValueError as e:
                    got = f"ValueError: {e}"
            lines.append(f"attr {fn}() under {var}={v!r} = {got!r}")
    record("vae *_from_env", lines)


def clip_record():
    from oracle import clip_ref as CR
    from seva.modules import conditioner as Cd
    p = Cd.ViTParams(width=320, layers=2, embed_dim=64)
    with environment({}):
        cond = Cd.CLIPConditioner(p, random_init=True)
        Cd.load_open_clip(cond.module, synth.synth_state_dict(CR.vit_shapes(320, 2, 14, 224, 1280, 64), 5))
        eng = cond.engine()
        inp = {"x": torch.zeros(2, 3, 300, 260)}
        lines = attribute_lines(eng) + tensor_lines("W", eng.W)
        lines += traced(lambda: eng.encode(inp["x"]), lambda: [("in", inp), ("W", eng.W), ("arena", eng.arena.bufs)])
        lines += [f"arena {k}" for k in eng.arena.bufs]
    record("clip encode", lines)


# ------------------------------------------------------------------------------------------------------------------ direct operator calls
def case_tensors(c, kc):
    """tensors of a case of tests/kernel_cases.py, in the shapes tests/test_kernel_coverage_gpu.py gives them (contents unused)"""
    M, N, K = kc.problem(c)
    NO = N // 2 if c.geglu else N
    dt = U8 if c.prec == "e4m3" else F16
    shapes = {"bias": ((N,), F32), "row_add": (((M + max(c.rpg, 1) - 1) // max(c.rpg, 1), N), F32), "residual": ((M, N), F32),
              "out_f32": ((M, NO), F32), "out_f16": ((M, 2 * NO if c.kind == "split_out" else NO), F16), "out_f8": ((M, NO), U8),
              "ch_stats": (ops.channel_stats_shape(M, N), F32), "w_exp": ((N,), U8), "a2": ((M, c.k2), F16)}
    if c.kind in kc.GEMM_KINDS:
        shapes.update(a=((M, K), dt), w=((N, K), dt))
    else:
        n, ih, iw, cin, cout = c.shape
        shapes.update(x=((n, ih, iw, cin), dt), w=((4, cout, 4 * cin), F16) if c.kind in ("phases", "phases128") else ((cout, K), dt))
    t = {k: torch.empty(shapes[k][0], dtype=shapes[k][1]) for k in kc.tensors_needed(c) if k != "splitk_ws"}
    if "splitk_ws" in c.ops:
        t["splitk_ws"] = ops.splitk_workspace(M, N, CPU)
    if c.kind in kc.CONV_KINDS:
        for k in ("residual", "out_f32", "out_f16", "out_f8"):
            if k in t:
                t[k] = t[k].view(c.shape[0], M // c.shape[0], -1)
    return t


def operator_records():
    import kernel_cases as kc
    lines = []
    for c in kc.CASES:
        t = case_tensors(c, kc)
        lines.append(f"case {c.id}")
        lines += traced(lambda: kc.launch(ops, c, t), lambda: [("t", t)])
    assert len(kc.CASES) >= 221
    record(f"ops: the {len(kc.CASES)} cases of tests/kernel_cases.py", lines)

    def e(*shape, dtype=F16):
        return torch.empty(shape, dtype=dtype)

    lines = []
    M, c = 96, 64
    t = {"a": e(M, c), "w1": e(8 * c, c), "b1": e(8 * c, dtype=F32), "w2": e(c, 4 * c), "b2": e(c, dtype=F32), "res": e(M, c, dtype=F32),
         "o32": e(M, c, dtype=F32), "o16": e(M, 2 * c)[:, :c], "x": e(M, c, dtype=F32), "g": e(c, dtype=F32), "be": e(c, dtype=F32),
         "a8": e(M, 128, dtype=U8), "w18": e(8 * c, 128, dtype=U8), "w1e": e(8 * c, dtype=U8), "w28": e(c, 4 * c, dtype=U8),
         "w2e": e(c, dtype=U8)}
    sp = lambda: [("t", t)]  # noqa: E731
    lines += traced(lambda: ops.ff_fused(t["a"], t["w1"], t["b1"], t["w2"], t["b2"], residual=t["res"], out_f32=t["o32"], out_f16=t["o16"]), sp)
    lines += traced(lambda: ops.ff_fused(None, t["w1"], t["b1"], t["w2"], t["b2"], out_f32=t["o32"], ln_x=t["x"], ln_gamma=t["g"],
                                         ln_beta=t["be"], ln_eps=1e-6), sp)
    lines += traced(lambda: ops.ff_fused_fp8(t["a8"], t["w18"], t["w1e"], t["b1"], t["w28"], t["w2e"], t["b2"], residual=t["res"],
                                             out_f32=t["o32"], out_f16=t["o16"]), sp)
    lines += traced(lambda: ops.ff_fused_fp8(None, t["w18"], t["w1e"], t["b1"], t["w28"], t["w2e"], t["b2"], out_f16=t["o16"], ln_x=t["x"],
                                             ln_gamma=t["g"], ln_beta=t["be"]), sp)
    nb0, nb1, heads, lq, lk = 2, 3, 2, 40, 56
    ch = 64 * heads
    t = {"q": e(nb0 * nb1 * lq, ch), "kv": e(nb0 * nb1 * lk, 2 * ch), "out": e(nb0 * nb1 * lq, ch),
         "sws": e(ops.attention_split_workspace_numel(nb0 * nb1, heads, lq), dtype=F32),
         "v8": e(ops.v_fp8_workspace_numel(nb0 * nb1, heads, lk), dtype=U8)}
    geo = dict(nb0=nb0, nb1=nb1, heads=heads, lq=lq, lk=lk, q_strides=(nb1 * lq * ch, lq * ch, ch),
               k_strides=(nb1 * lk * 2 * ch, lk * 2 * ch, 2 * ch), o_strides=(nb1 * lq * ch, lq * ch, ch))
    k, v = t["kv"][:, :ch], t["kv"][:, ch:]
    lines += traced(lambda: ops.attention(t["q"], k, v, t["out"], **geo), sp)
    lines += traced(lambda: ops.attention(t["q"], k, v, t["out"], scale=0.25, **geo), sp)
    lines += traced(lambda: ops.attention(t["q"], k, v, t["out"], q_prescaled=True, **geo), sp)
    lines += traced(lambda: ops.attention(t["q"], k, v, t["out"], q_prescaled=True, split_ws=t["sws"], **geo), sp)
    lines += traced(lambda: ops.attention(t["q"], k, v, t["out"], split_ws=t["sws"], **geo), sp)
    lines += traced(lambda: ops.quantize_v_fp8(v, t["v8"], nb0=nb0, nb1=nb1, heads=heads, lk=lk, k_strides=geo["k_strides"]), sp)
    lines += traced(lambda: ops.attention_pv8(t["q"], k, t["v8"], t["out"], **geo), sp)
    lines += traced(lambda: ops.attention_pv8(t["q"], k, t["v8"], t["out"], split_ws=t["sws"], **geo), sp)
    record("ops: fused feed-forwards and attention", lines)


# ------------------------------------------------------------------------------------------------------------------ sampler
SAMPLER_OPS = ("scale_rows", "add_noise", "replace_blend", "denoiser_combine", "cfg_combine", "cfg_euler", "euler_step", "cfg_multistep",
               "cfg_rescale")
SAMPLER_T, SAMPLER_STEPS = 4, 3
# the opt-in modes: the 10-step case of tests/test_guidance_cpu.py -- cache_interval 3 at depth 2 and an interval that guides steps 3..7
# give F S S F S S F S F F over unguided, guided, unguided: every step kind occurs
MODE_STEPS, MODE_CACHE, MODE_INTERVAL, MODE_RESCALE = 10, dict(cache_interval=3, cache_levels=2), (3.0, 25.0), 0.7
NETWORK_CALLS = []  # (rows, rows of a guided call, shallow depth) of every network call of the opt-in sampler records, for the coverage table


@contextlib.contextmanager
def keeping_arguments(kept, host):
    """While active, every tensor handed to an operator of the sampler stays alive in `kept`, the step's own temporaries included:
    a freed block could be handed out again, and an ordinal would no longer mean identity.  The per-frame vectors among them (host
    math: sigmas, noise scales, guidance scales, solver coefficients) are written to `host` by value."""
    real = {name: getattr(ops, name) for name in SAMPLER_OPS}

    def wrap(name, fn):
        def call(*a, **kw):
            ts = [t for t in (*a, *kw.values()) if isinstance(t, torch.Tensor)]
            kept.extend(ts)
            host.append(f"host {name} " + json.dumps([t.tolist() for t in ts if t.ndim == 1]))
            return fn(*a, **kw)
        return call

    for name, fn in real.items():
        setattr(ops, name, wrap(name, fn))
    try:
        yield
    finally:
        for name, fn in real.items():
            setattr(ops, name, fn)


def analytic_denoiser(xx, ss, cc):
    """[uncond ; cond] halves of D = mu (1 - k) + x k, k = 1 / (1 + sigma^2): plain torch, no operator call"""
    n = xx.shape[0] // 2
    k = (1.0 / (1.0 + ss * ss)).view(-1, 1, 1, 1)
    mu = torch.cat([torch.full((n,), 0.3), torch.full((n,), -0.2)]).view(-1, 1, 1, 1)
    return mu * (1 - k) + xx * k


def depth_recording_denoiser(host):
    """A network of any batch that writes its rows and the depth the sampler asked for (`_native.shallow_network`) into the record:
    a shallow step differs from a full one, an unguided step (n rows) from a guided one (2n)."""
    def denoiser(xx, ss, cc):
        L = nv.network_shallow_levels()
        host.append(f"host network rows={xx.shape[0]} shallow_levels={L}")
        NETWORK_CALLS.append((xx.shape[0], 2 * SAMPLER_T, L))
        return torch.zeros_like(xx)
    return denoiser


def sampler_guider(S, kind):
    """(guider, guider_kwargs)"""
    T = SAMPLER_T
    mask = torch.zeros(T, dtype=torch.bool)
    mask[0] = True
    views = {"c2w": synth.orbit_c2w(T), "K": synth.default_K(T), "input_frame_mask": mask}
    if kind == "vanilla":
        return S.VanillaCFG(), {}
    if kind == "multiview":
        return S.MultiviewCFG(1.2), views
    if kind == "temporal":
        return S.MultiviewTemporalCFG(T, 1.2), views

    class PlainGuider:  # no `frame_scale`: the sampler calls it, then the plain update
        def prepare_inputs(self, x, s, c, uc):
            return S.VanillaCFG().prepare_inputs(x, s, c, uc)

        def __call__(self, x, sigma, scale):
            return S.ConstantGuidance()(*x.chunk(2), scale)

    return PlainGuider(), {}


SAMPLER_ATTRS = ("solver", "cache_interval", "cache_levels", "guidance_interval", "guidance_rescale")


def sampler_record(solver, kind, s_churn=0.0, env=None, **opts):
    """Default options: three steps.  With `env` or sampler options: `MODE_STEPS` steps behind the depth-recording network, and the
    record states the options the sampler resolved."""
    from seva import sampling as S
    guider, guider_kwargs = sampler_guider(S, kind)
    modes = env is not None or bool(opts)
    with environment(env or {}):
        sm = S.EulerEDMSampler(S.DDPMDiscretization(), guider, num_steps=MODE_STEPS if modes else SAMPLER_STEPS, verbose=False,
                               device="cpu", s_churn=s_churn, solver=solver, **opts)
        sm.noise_fn = torch.zeros_like
        inp = {"x": torch.zeros(SAMPLER_T, 4, 8, 8)}
        kept, host = [], []
        net = depth_recording_denoiser(host) if modes else analytic_denoiser

        def run():
            with keeping_arguments(kept, host):
                return sm(net, inp["x"], 2.0, {}, {}, **guider_kwargs), kept

        lines = traced(run, lambda: [("in", inp), ("ms", {"den": sm._ms_den})])
    name = f"sampler {solver} {kind} s_churn={s_churn}"
    if modes:
        name += f" {env_tag(env or {}, **opts)} steps={MODE_STEPS}"
        lines = ["attr " + json.dumps({k: getattr(sm, k) for k in SAMPLER_ATTRS})] + lines
    record(name, lines + host)


def denoiser_record():
    from seva import sampling as S
    n = 2 * SAMPLER_T
    inp = {"x": torch.zeros(n, 4, 8, 8), "sigma": torch.full((n,), 9.3527), "replace": torch.zeros(n, 5, 8, 8)}
    kept, host = [], []

    def run():
        with keeping_arguments(kept, host):
            den = S.DiscreteDenoiser(S.DDPMDiscretization(), num_idx=1000, device="cpu")
            return den(lambda x, t, cond: 0.5 * x, inp["x"], inp["sigma"], {"replace": inp["replace"]}), kept

    lines = traced(run, lambda: [("in", inp)])
    record("sampler DiscreteDenoiser with replace", lines + host)


def sampler_configurations():
    from seva import sampling as S
    S._need_gpu = lambda *a: None
    for kind in ("vanilla", "multiview", "temporal", "plain"):
        sampler_record("euler", kind)
        sampler_record("euler", kind, s_churn=0.5)
        sampler_record("dpmpp2m", kind)
    denoiser_record()
    iv_env = "%g,%g" % MODE_INTERVAL
    for solver in S.SOLVERS:
        # each mode alone and all three together, as arguments
        sampler_record(solver, "multiview", cache_interval=3)
        sampler_record(solver, "multiview", guidance_interval=MODE_INTERVAL)
        sampler_record(solver, "multiview", guidance_rescale=MODE_RESCALE)
        sampler_record(solver, "multiview", **MODE_CACHE, guidance_interval=MODE_INTERVAL, guidance_rescale=MODE_RESCALE)
        # each through its variable; the depth's variable with and without the interval's (without: the mode stays off)
        sampler_record(solver, "multiview", env={"SEVA_CACHE_INTERVAL": 3})
        sampler_record(solver, "multiview", env={"SEVA_GUIDANCE_INTERVAL": iv_env})
        sampler_record(solver, "multiview", env={"SEVA_GUIDANCE_RESCALE": MODE_RESCALE})
        sampler_record(solver, "multiview", env={"SEVA_CACHE_INTERVAL": 3, "SEVA_CACHE_LEVELS": 2})
        sampler_record(solver, "multiview", env={"SEVA_CACHE_LEVELS": 2})
        # the depth's variable is not read where the interval is an argument; an explicit argument wins over every variable
        sampler_record(solver, "multiview", env={"SEVA_CACHE_LEVELS": 2}, cache_interval=3)
        sampler_record(solver, "multiview", env={"SEVA_CACHE_INTERVAL": 2, "SEVA_GUIDANCE_INTERVAL": "1,2", "SEVA_GUIDANCE_RESCALE": 1,
                                                 "SEVA_SOLVER": "euler" if solver == "dpmpp2m" else "dpmpp2m"},
                       **MODE_CACHE, guidance_interval=MODE_INTERVAL, guidance_rescale=MODE_RESCALE)
        # SEVA_SOLVER instead of the argument
        sampler_record(None, "multiview", env={"SEVA_SOLVER": solver}, **MODE_CACHE)
        # a guider without `frame_scale` under the interval (full and shallow)
        sampler_record(solver, "plain", guidance_interval=MODE_INTERVAL)
        sampler_record(solver, "plain", guidance_interval=MODE_INTERVAL, **MODE_CACHE)
    sampler_record(None, "multiview", env={"SEVA_SOLVER": ""}, guidance_interval=MODE_INTERVAL)  # empty: unset
    sampler_record("euler", "multiview", s_churn=0.5, guidance_interval=MODE_INTERVAL)
    sampler_record("euler", "multiview", s_churn=4.0, guidance_interval=MODE_INTERVAL, guidance_rescale=MODE_RESCALE, **MODE_CACHE)


# ------------------------------------------------------------------------------------------------------------------ drivers
DRIVER_VIEWS, DRIVER_T, DRIVER_STEPS = 43, 21, 3  # tests/test_pipeline_cpu.py, test_step_cache_cpu.py, test_guidance_cpu.py: their sizes
DRIVER_SEEN = {"per-pass pair": 0, "keep_own": 0}


class StandInAE:
    """cheap deterministic maps in place of the VAE: (k,4,h,w) -> (k,3,h,w) and back"""

    def decode(self, z):
        return torch.tanh(z[:, :3] * 0.5 + 0.1 * z[:, 3:4])

    def encode(self, x):
        return torch.cat([x * 1.5, x.mean(1, keepdim=True)], 1)


@contextlib.contextmanager
def emulated_operators():
    """The drivers compute: `seva.ops` becomes the torch emulation of tests/ (fake_ops.py, and the two newer sampler operators)."""
    import fake_guidance_ops
    import fake_ops
    from seva import geometry
    from test_solver_dpmpp2m_cpu import _fake_cfg_multistep
    new = {name: getattr(fake_ops, name) for name in dir(fake_ops)
           if not name.startswith("_") and callable(getattr(fake_ops, name)) and hasattr(ops, name)}
    new.update(cfg_multistep=_fake_cfg_multistep, cfg_rescale=fake_guidance_ops.cfg_rescale)
    saved = {name: getattr(ops, name) for name in new}
    saved_device = geometry._compute_device
    for name, fn in new.items():
        setattr(ops, name, fn)
    geometry._compute_device = lambda *a: CPU
    try:
        yield
    finally:
        for name, fn in saved.items():
            setattr(ops, name, fn)
        geometry._compute_device = saved_device


def sha(t):
    return hashlib.sha256(t.detach().contiguous().view(-1).view(U8).numpy().tobytes()).hexdigest()


def driver_record(name, views=False, env=None, **kw):
    """One run of `run_trajectory` (`views`: `run_views`) on one process: the plan, what every window's sampler was built with, the
    timers' keys, and the results by SHA-256."""
    from seva import pipeline
    from test_pipeline_cpu import _fake_net, _scene
    c2ws, Ks, lat, tok = _scene(DRIVER_VIEWS)
    built, timers = [], {}

    def hook(sm):
        built.append([type(sm.guider).__name__, getattr(sm.guider, "num_frames", None)] + [getattr(sm, k) for k in SAMPLER_ATTRS])

    with environment(env or {}):
        res = (pipeline.run_views if views else pipeline.run_trajectory)(
            _fake_net, lat, c2ws, Ks, [0], clip_token=tok, T=DRIVER_T, num_steps=DRIVER_STEPS, seed=23, device="cpu",
            sampler_hook=hook, timers=timers, **kw)
    plan = res["plan"]
    wins = plan.pass1 + plan.pass2
    assert len(built) == len(wins), (name, len(built), len(wins))  # one process: every window, in plan order
    lines = [f"plan pass1={len(plan.pass1)} pass2={len(plan.pass2)} serial={plan.pass1_serial} T1={plan.T1} T2={plan.T2}",
             "plan global_index " + json.dumps([w.global_index for w in wins]), "plan anchors " + json.dumps(plan.anchor_ids)]
    lines += [f"window pass={w.pass_id} index={w.index} slots={len(w.slot_frame)} " + json.dumps(b) for w, b in zip(wins, built)]
    lines.append("timers " + json.dumps(sorted(timers)))
    lines.append("windows " + json.dumps([t[:2] for t in timers["windows"]]))
    lines.append("result " + json.dumps(sorted(res)) + " frame_ids " + sha(torch.tensor(res["frame_ids"])))
    lines.append(f"latents {list(res['latents'].shape)} {sha(res['latents'])}")
    lines += [f"anchor_latent {fid} {sha(z)}" for fid, z in res["anchor_latents"].items()]
    if "rgb" in res:
        lines.append(f"rgb {list(res['rgb'].shape)} {sha(res['rgb'])}")
    opts1, opts2 = ({json.dumps(b[2:]) for w, b in zip(wins, built) if w.pass_id == p} for p in (1, 2))
    DRIVER_SEEN["per-pass pair"] += bool(opts1 and opts2 and opts1 != opts2)
    # `keep_own`: a frame's output is its own sample, while later windows saw the latent that came back from the hand-off
    DRIVER_SEEN["keep_own"] += any(not torch.equal(res["latents"][fid], z) for fid, z in res["anchor_latents"].items()
                                   if not plan.pass2)
    record(f"driver {name}", lines)


def driver_configurations():
    with emulated_operators():
        driver_record("default")
        driver_record("refine_anchors=False", refine_anchors=False)
        driver_record("first_pass_strategy=gt", first_pass_strategy="gt")
        driver_record("cfg=(3.0, 2.0) guider=(1, 2)", cfg=(3.0, 2.0), guider=(1, 2))
        driver_record("solver=dpmpp2m", solver="dpmpp2m")
        driver_record("cache_interval=(3, 2) cache_levels=(1, 2)", cache_interval=(3, 2), cache_levels=(1, 2))
        driver_record("guidance_interval=((0.5, 3), None) guidance_rescale=(0.0, 0.5)",
                      guidance_interval=((0.5, 3), None), guidance_rescale=(0.0, 0.5))
        driver_record("guidance_interval=(0.3, 5)", guidance_interval=(0.3, 5))
        driver_record("guidance_interval=('0.3,5', (0.5, 3))", guidance_interval=("0.3,5", (0.5, 3)))
        driver_record("guidance_interval=((0.3, 5), None) guidance_rescale=(None, 0) GUIDANCE_INTERVAL=0.5,3 GUIDANCE_RESCALE=0.7",
                      env={"SEVA_GUIDANCE_INTERVAL": "0.5,3", "SEVA_GUIDANCE_RESCALE": "0.7"},
                      guidance_interval=((0.3, 5), None), guidance_rescale=(None, 0))
        driver_record("handoff=rgb", handoff="rgb", ae=StandInAE())
        driver_record("handoff=rgb run_views", views=True, handoff="rgb", ae=StandInAE())
        driver_record("anchor_ids=[7, 14, 21, 28, 35, 42]", anchor_ids=[7, 14, 21, 28, 35, 42])
        driver_record("run_views", views=True)
        driver_record("run_views chunk_strategy=gt-nearest", views=True, chunk_strategy="gt-nearest")


# ------------------------------------------------------------------------------------------------------------------ coverage
def coverage():
    def field(rec, f):
        return next((v for g, _, v in rec if g == f), None)

    def seen(sym, pred=lambda r: True):
        return sum(1 for s, r in RAW if s == sym and pred(r))

    gemms = ("seva_gemm_f16", "seva_gemm_f16_split_out", "seva_gemm_fp8")

    def gemm(pred):
        return sum(seen(s, pred) for s in gemms)

    attn = ("seva_attention_f16", "seva_attn_quant_v_fp8", "seva_attention_pv8")
    table = {s: seen(s) for s in gemms + ("seva_ff_fused_f16", "seva_ff_fused_fp8") + attn}
    table["attention split_ws"] = sum(seen(s, lambda r: field(r, "split_ws")) for s in attn)
    table["gemm a2"] = gemm(lambda r: field(r, "a2"))
    for u in (1, 2, 4):
        table[f"conv upsample={u}"] = gemm(lambda r: field(r, "mode") == 1 and field(r, "upsample") == u)
    table["conv stride=2 pad_br_only"] = gemm(lambda r: field(r, "stride") == 2 and field(r, "pad_br_only") == 1)
    table["conv out_f8"] = gemm(lambda r: field(r, "mode") == 1 and field(r, "out_f8"))
    for f in ("w_exp", "splitk_ws", "ch_stats", "alg_K"):
        table[f"gemm {f}"] = gemm(lambda r: field(r, f))
    for f in ("stats1", "stats2", "raw_f16", "out_f8", "split_out_f16", "split_raw_f16"):
        table[f"groupnorm {f}"] = seen("seva_groupnorm_f16", lambda r: field(r, f))
    for s in ("seva_layernorm_f16", "seva_layernorm_fp8", "seva_layernorm_f16_split"):
        table[s] = seen(s)
    for s in ("seva_cfg_euler_f32", "seva_euler_step_f32", "seva_replace_blend_f32"):
        table[s] = seen(s)
    table["shallow call, entry with stats"] = len(SHALLOW_WITH_STATS)  # a shallow call whose entering tensor came with statistics
    table["seva_cfg_multistep_f32 scale"] = seen("seva_cfg_multistep_f32", lambda r: field(r, "arg2"))
    table["seva_cfg_multistep_f32 no scale"] = seen("seva_cfg_multistep_f32", lambda r: not field(r, "arg2"))
    table["seva_cfg_rescale_f32"] = seen("seva_cfg_rescale_f32")
    table["sampler: shallow step"] = sum(1 for rows, guided_rows, L in NETWORK_CALLS if L)
    table["sampler: unguided step"] = sum(1 for rows, guided_rows, L in NETWORK_CALLS if rows != guided_rows)
    table["sampler: unguided shallow step"] = sum(1 for rows, guided_rows, L in NETWORK_CALLS if L and rows != guided_rows)
    table["driver: per-pass pair"] = DRIVER_SEEN["per-pass pair"]
    table["driver: keep_own branch"] = DRIVER_SEEN["keep_own"]
    print("\ncoverage (recorded calls over all configurations)")
    for k, v in table.items():
        print(f"  {k:32s} {v:7d}")
    return [k for k, v in table.items() if not v]


def kv_split_check():
    """the 96 x 96 input of the default engine: three K/V-split attention launches (joint key length 3 * 48 * 48 = 6912 >= 6144)"""
    rec = RECORDS["unet[tiny] default"].split("input T3_96x96_lc1\n")[1]
    n = sum(1 for ln in rec.splitlines() if ln.startswith("call seva_attention_f16 ") and '["split_ws", 0]' not in ln)
    print(f"K/V-split attention launches of the default engine at 96 x 96: {n}")
    return n == 3


unet_configurations()
vae_configurations()
clip_record()
operator_records()
sampler_configurations()
driver_configurations()
missing = coverage()
split_ok = kv_split_check()
digests = {name: hashlib.sha256(text.encode()).hexdigest() for name, text in RECORDS.items()}
if args.out:
    os.makedirs(args.out, exist_ok=True)
    for i, (name, text) in enumerate(RECORDS.items()):
        with open(os.path.join(args.out, f"{i:03d}.txt"), "w") as f:
            f.write(f"# {name}\n{text}")
    with open(os.path.join(args.out, "digests.txt"), "w") as f:
        f.writelines(f"{d}  {name}\n" for name, d in digests.items())
status = 0
if missing:
    print("never seen:", ", ".join(missing))
    status = 1
if not split_ok:
    status = 1
if args.against:
    other = dict(reversed(ln.rstrip("\n").split("  ", 1)) for ln in open(args.against))
    print(f"\n{'other run':20s}  {'this run':20s}  configuration")
    differ = 0
    for name in list(other) + [n for n in digests if n not in other]:
        a, b = other.get(name, "-"), digests.get(name, "-")
        differ += a != b
        print(f"{a[:20]:20s}  {b[:20]:20s}  {'   ' if a == b else '!= '}{name}")
    print(f"{len(digests)} configurations, {differ} differ")
    status = status or int(differ > 0)
sys.exit(status)
