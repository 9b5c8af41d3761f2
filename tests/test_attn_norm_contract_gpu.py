"""The two promises of the C-ABI (include/seva_hip.h) for the attention, normalisation and elementwise half of the hot path, the
counterpart of test_gemm_contract_gpu.py.

A. Batch invariance.  A sample's result does not depend on the launch it is part of: frame-sliced execution, graph replay, the CFG
   split over two ranks and sharded == single-process all compare bits.  Every case runs a small launch and a large one whose
   leading samples / rows are the same RANDOM data (integer data cannot see a change of reduction order) and asserts equality of the
   raw bits (f16 as int16, f32 as int32, e4m3 as bytes).
B. Strides, guards, poison.  Every operand is addressed through its strides / pitch; nothing outside the logical output is written
   (outputs are views into larger buffers pre-filled with NaN / 0x7F bytes, checked bit-unchanged); nothing outside the logical
   inputs is USED (rows >= lq / lk, pitch gaps, gaps between samples, columns >= cols hold NaN inside buffers this file allocates
   with whole tiles of room, and the result must be finite and bit-equal to the same launch with zeros there).

fp64 references are computed on exactly the operands the kernel sees; the bounds are the ones the project already asserts for the
same kernel on the same input distribution (test_ops_gpu.py, test_fp8_gpu.py, test_clip_gpu.py, test_attention_fp8_gpu.py).  The one
new bound, the fp32-output LayerNorm, is 4x the rel-L2 error of torch's own fp32 F.layer_norm against fp64 on the same input
(another summation order over up to 1280 terms); both figures are printed.

Case ids and the kernel instantiation their shapes steer to (csrc/attention.hip seva_attention_f16, csrc/attention_fp8.hip,
csrc/clip.hip, csrc/norm.hip, csrc/elementwise.hip); a kernel trace of this file (rocprofv3 --kernel-trace --stats) lists them:

  temporal_1wave        attn_kernel<1, 32>  (lq <= 32), tokens = frames, batch = (b, pixel), strided `(b t) s c` layout
  cross_plain_scale     attn_kernel<4, 64>, q not pre-scaled (the cross-attention launches)
  frame_4wave           attn_kernel<4, 64>, q pre-scaled, 32 < lq < 2048
  frame_attn16          attn16_kernel<64>  (lq >= 2048); 21 query blocks per (sample, head): grids with nb & 7 = 5, 7, 0 (XCD remap)
  frame_attn2           attn2_kernel<64>   (knob attn_two = 1, lq >= 512)
  joint_split           attn16_kernel<64, true> + attn_combine_kernel  (lk >= 6144 and a workspace)
  joint_split_forced    the same with knob attn_split = 3: 21 key tiles in splits of 7, a ragged last tile in the last split
  frame_attn16_unsplit  attn16_kernel<64> at lk >= 6144 WITHOUT a workspace: the per-frame regime of the engine passes none, so at the
                        non-square latents 72x96 / 96x72 (6912 tokens) and 72x128 (9216) one workgroup per query block walks every key
  pv8                   quant_v_fp8_kernel + pv8_kernel<false> (5184 keys) / pv8_kernel<true> + attn_combine_kernel (>= 6144 keys)
  pv8_unsplit_no_ws     seva_attention_pv8 at >= 6144 keys with split_ws absent: nsplit is still computed as 2, but the split branch
                        needs the workspace, so the launch falls through to the unsplit pv8_kernel<false> over all 128-key steps
  small                 attn_small_kernel (CLIP: L = 257, head dim 80); batch 1 -> qchunks 8, batch 21 -> qchunks 1
  layernorm c<C>-<out>  layernorm_kernel<NV, 1, OUT> (rows < 65536) against <NV, 4, OUT> (rows >= 65536); NV = 2, 5, 10, 20 for
                        C = 64, 320, 640, 1280; OUT = 0 f16, 1 e4m3, 2 fp32
  groupnorm *           gn_stats_kernel + gn_finalize_kernel + gn_apply_kernel<false> (plain), <true, true> (6-component modulation),
                        <true> (dense4: 4 components), <true, true, true> (splitraw), <false, false, true> (splitout)
  softmax_rows *        softmax_rows_kernel
  elementwise <op>-big  every kernel of elementwise.hip above the 8192 x 256 grid cap (the grid-stride loop runs), -odd: sizes that
                        are not multiples of 4, hw = 1
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from conftest import rel_l2

U8, F16, F32, F64 = torch.uint8, torch.float16, torch.float32, torch.float64
QK_C = 0.125 * 1.4426950408889634
LN2 = math.log(2.0)
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from seva import _native
    _native.load()
    return torch.device("cuda:0")


def _randn(shape, dev, seed, scale=1.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(shape, generator=g, device=dev) * scale


def _bits(t):
    return t.view({F16: torch.int16, F32: torch.int32, U8: U8}[t.dtype])


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _pattern(dtype):
    return 0x7F if dtype == U8 else NAN


def _guarded(shape, dtype, dev):
    return torch.full(shape, _pattern(dtype), dtype=dtype, device=dev)


def _outside_untouched(buf, *views):
    """Every element of the freshly allocated guard buffer `buf` outside `views` (views into it) still holds the guard's bits."""
    chk = buf.clone()
    for v in views:
        torch.as_strided(chk, v.size(), v.stride(), v.storage_offset()).fill_(_pattern(buf.dtype))
    return bool((_bits(chk) == _bits(_guarded((1,), buf.dtype, buf.device))).all())


def _close_fp8(got_u8, ref_f32):
    """The comparison of test_fp8_gpu.py::_close_fp8: e4m3 bytes equal torch's cast of the reference except where fp32 arithmetic
    differences cross a rounding tie (> 99.5 % identical, every element within one e4m3 step)."""
    from seva import ops
    got = got_u8.view(torch.float8_e4m3fn).float()
    want = ops.to_fp8(ref_f32).view(torch.float8_e4m3fn).float()
    same = (got == want).float().mean().item()
    ulp = torch.maximum(ref_f32.abs() * 2.0 ** -3, torch.tensor(2.0 ** -9, device=ref_f32.device))
    assert same > 0.995 and bool(((got - ref_f32).abs() <= ulp).all()), same
    return same


# ------------------------------------------------------------------------------------------------------------------------------
# attention: one problem = q / k / v in separate flat f16 buffers
# ------------------------------------------------------------------------------------------------------------------------------
class _Attn:
    """q, k, v (and every output) are flat f16 buffers laid out [nb0][L + gap][nb1][pitch] plus `tail` token rows, pitch = 64 H + pad:
    token stride nb1 * pitch, inner batch stride pitch, outer batch stride (L + gap) * nb1 * pitch.  nb1 = 1 is the per-frame layout
    ([B][L][C]), nb1 > 1 the temporal `(b t) s c` one.  Everything that is not a logical q / k / v element (rows >= L of a sample, the
    columns behind 64 H, the tail) holds `poison`.  A launch may take the leading nb0 x nb1 samples and H heads from head h0 on."""

    def __init__(self, dev, nb0, nb1, H, lq, lk, *, pad=0, gap=0, seed=1, poison=NAN, prescaled=True):
        self.dev, self.nb0, self.nb1, self.H, self.lq, self.lk, self.pre = dev, nb0, nb1, H, lq, lk, prescaled
        P = self.pitch = 64 * H + pad
        tail = 256 if nb1 == 1 else 32  # whole tiles of room behind the last sample (256-row query blocks; 32 for the 1-wave kernel)

        def strides(L):
            return ((L + gap) * nb1 * P, P, nb1 * P)

        def buf(L, sd, scale):
            st = strides(L)
            b = torch.full((nb0 * st[0] + tail * nb1 * P,), poison, dtype=F16, device=dev)
            data = (_randn((nb0, L, nb1, 64 * H), dev, sd) * scale).half()
            torch.as_strided(b, data.shape, (st[0], st[2], st[1], 1)).copy_(data)
            return b

        self.qs, self.ks = strides(lq), strides(lk)
        self.os = self.qs
        self.q = buf(lq, seed, QK_C if prescaled else 1.0)
        self.k, self.v = buf(lk, seed + 1, 1.0), buf(lk, seed + 2, 1.0)

    @staticmethod
    def _view(b, st, L, nb0, nb1, H, h0):  # [nb0, nb1, H, L, 64]
        return torch.as_strided(b, (nb0, nb1, H, L, 64), (st[0], st[1], 64, st[2], 1), 64 * h0)

    def oview(self, out, nb0, nb1, H, h0=0):
        return self._view(out, self.os, self.lq, nb0, nb1, H, h0)

    def run(self, nb0, nb1, H, h0=0, *, swap=False, ws=None, pv8=False):
        """One launch into a fresh NaN buffer of the output layout; returns the buffer.  swap: the same samples with the roles of
        (nb0, sb0) and (nb1, sb1) exchanged (the kernels' b0 / b1 decode)."""
        from seva import ops
        out = torch.full_like(self.q, NAN)
        off = 64 * h0
        a0, a1 = (nb1, nb0) if swap else (nb0, nb1)
        sw = (lambda s: (s[1], s[0], s[2])) if swap else (lambda s: s)
        kw = dict(nb0=a0, nb1=a1, heads=H, lq=self.lq, lk=self.lk, q_strides=sw(self.qs), k_strides=sw(self.ks), o_strides=sw(self.os))
        if ws is not None:
            ws.fill_(NAN)  # stale partials must not leak
        if pv8:
            vws = torch.full((ops.v_fp8_workspace_numel(a0 * a1, H, self.lk),), 0x7F, dtype=U8, device=self.dev)
            ops.quantize_v_fp8(self.v[off:], vws, nb0=a0, nb1=a1, heads=H, lk=self.lk, k_strides=kw["k_strides"])
            ops.attention_pv8(self.q[off:], self.k[off:], vws, out[off:], split_ws=ws, **kw)
        else:
            ops.attention(self.q[off:], self.k[off:], self.v[off:], out[off:], scale=0.125, q_prescaled=self.pre, split_ws=ws, **kw)
        torch.cuda.synchronize()
        o = self.oview(out, nb0, nb1, H, h0)
        assert torch.isfinite(o).all(), "non-finite output"
        assert _outside_untouched(out, o), "written outside the logical output"
        return out

    def operands(self, nb0, nb1, H, h0=0):
        return (self._view(self.q, self.qs, self.lq, nb0, nb1, H, h0), self._view(self.k, self.ks, self.lk, nb0, nb1, H, h0),
                self._view(self.v, self.ks, self.lk, nb0, nb1, H, h0))

    def ref(self, nb0, nb1, H, h0=0):
        """fp64 softmax(q k^T) v of the launch on the f16 operands, [nb0, nb1, H, lq, 64]; chunked over samples and query rows"""
        q, k, v = (t.reshape(-1, t.shape[-2], 64) for t in self.operands(nb0, nb1, H, h0))
        out = torch.empty(q.shape, dtype=F64, device=self.dev)
        rows = min(self.lq, 1024)
        nb = max(1, (1 << 24) // (rows * self.lk))
        c = LN2 if self.pre else 0.125
        for b in range(0, q.shape[0], nb):
            kd, vd = k[b:b + nb].double(), v[b:b + nb].double()
            for r in range(0, self.lq, rows):
                s = q[b:b + nb, r:r + rows].double() @ kd.transpose(-1, -2) * c
                out[b:b + nb, r:r + rows] = torch.softmax(s, -1) @ vd
        return out.view(nb0, nb1, H, self.lq, 64)

    def ref_pv8(self, nb0, nb1, H, h0, rows):
        """pv8_kernel's own arithmetic in fp64 (tests/test_attention_fp8_cpu.py) on the query rows `rows`: [nb0 * nb1, H, len(rows), 64]"""
        from test_attention_fp8_cpu import pv8_reference, quantize_v_ref
        q, k, v = (t.reshape(-1, H, t.shape[-2], 64) for t in self.operands(nb0, nb1, H, h0))
        _, _, vhat = quantize_v_ref(v.permute(0, 2, 1, 3).cpu())  # [B, L, H, 64] -> dequantised [B, H, L, 64]
        return pv8_reference(q[:, :, rows], k, vhat.to(self.dev))


def _pv8_rows(lq, dev):
    g = torch.Generator().manual_seed(0)
    r = torch.randperm(lq, generator=g)[:192]
    return torch.unique(torch.cat([r, torch.arange(max(0, lq - 40), lq), torch.arange(min(40, lq))])).to(dev)


def _attn_error(P, out, cfg, pv8):
    """rel-L2 of the launch `cfg` = (nb0, nb1, H, h0) against fp64 (pv8: against the kernel's stated arithmetic on sampled rows)"""
    nb0, nb1, H, h0 = cfg
    got = P.oview(out, nb0, nb1, H, h0)
    if pv8:
        rows = _pv8_rows(P.lq, P.dev)
        return rel_l2(got.reshape(-1, H, P.lq, 64)[:, :, rows], P.ref_pv8(nb0, nb1, H, h0, rows))
    return rel_l2(got, P.ref(nb0, nb1, H, h0))


def _split_ws(P, nb0, nb1, H, dev):
    from seva import ops
    return torch.empty(ops.attention_split_workspace_numel(nb0 * nb1, H, P.lq, 4), device=dev)


# id, lq, lk, (nb0, nb1, H) of the large launch, small launches (nb0, nb1, H, h0), knobs, kind, bound of the fp64 comparison
# kinds: "pre" q pre-scaled (as the engine calls it), "plain" scale 0.125, "ws" pre-scaled + K/V-split workspace, "pv8", "pv8ws"
ATTN_A = [
    ("temporal_1wave-21x21", 21, 21, (2, 5184, 5), [(1, 81, 1, 0), (1, 5184, 5, 0), (2, 81, 5, 0), (2, 5184, 1, 3)], {}, "pre", 2e-3),
    ("cross_plain_scale-1296x21", 1296, 21, (5, 1, 5), [(1, 1, 5, 0), (5, 1, 1, 2)], {}, "plain", 2e-3),
    ("cross_plain_scale-5184x1", 5184, 1, (5, 1, 5), [(1, 1, 5, 0), (5, 1, 1, 4)], {}, "plain", 2e-3),
    ("frame_4wave-1296x1296", 1296, 1296, (42, 1, 20), [(1, 1, 1, 0), (1, 1, 5, 10), (1, 1, 20, 0), (42, 1, 1, 7)], {}, "pre", 2e-3),
    ("frame_4wave-324x324", 324, 324, (42, 1, 20), [(1, 1, 1, 0), (1, 1, 5, 15), (1, 1, 20, 0), (42, 1, 5, 5)], {}, "pre", 2e-3),
    ("frame_4wave-33x64", 33, 64, (42, 1, 20), [(1, 1, 1, 0), (1, 1, 5, 15), (1, 1, 20, 0), (42, 1, 5, 5)], {}, "pre", 2e-3),
    ("frame_attn16-5184x5184-batch", 5184, 5184, (8, 1, 1), [(1, 1, 1, 0), (3, 1, 1, 0)], {}, "pre", 1e-3),
    ("frame_attn16-5184x5184-heads", 5184, 5184, (1, 1, 5), [(1, 1, 1, 0), (1, 1, 1, 4)], {}, "pre", 1e-3),
    ("frame_attn2-5184x5184", 5184, 5184, (3, 1, 2), [(1, 1, 2, 0), (3, 1, 1, 1)], {"attn_two": 1}, "pre", 1e-3),
    ("frame_attn2-777x1300", 777, 1300, (3, 1, 2), [(1, 1, 2, 0), (3, 1, 1, 1)], {"attn_two": 1}, "pre", 1e-3),
    ("joint_split-6804x6804", 6804, 6804, (2, 1, 5), [(1, 1, 5, 0), (2, 1, 2, 0), (1, 1, 2, 3)], {}, "ws", 1e-3),
    ("joint_split_forced-2049x1300", 2049, 1300, (4, 1, 2), [(1, 1, 2, 0), (4, 1, 1, 1)], {"attn_split": 3}, "ws", 1e-3),
    # pv8: the bound of test_attention_fp8_gpu.py::test_kernel_does_the_stated_arithmetic (against the kernel's arithmetic in fp64)
    ("pv8-5184x5184", 5184, 5184, (1, 1, 5), [(1, 1, 1, 0), (1, 1, 1, 3)], {}, "pv8", 4e-3),
    ("pv8-6804x6804", 6804, 6804, (1, 1, 5), [(1, 1, 1, 0), (1, 1, 1, 3)], {}, "pv8ws", 4e-3),
    # the per-frame regime at the non-square latents: >= 6144 keys and NO workspace (unsplit kernels)
    ("frame_attn16_unsplit-6912x6912", 6912, 6912, (3, 1, 2), [(1, 1, 2, 0), (3, 1, 1, 1)], {}, "pre", 1e-3),
    ("frame_attn16_unsplit-9216x9216", 9216, 9216, (3, 1, 2), [(1, 1, 2, 0), (3, 1, 1, 1)], {}, "pre", 1e-3),
    ("pv8_unsplit_no_ws-6912x6912", 6912, 6912, (3, 1, 2), [(1, 1, 2, 0), (3, 1, 1, 1)], {}, "pv8", 4e-3),
    ("pv8_unsplit_no_ws-9216x9216", 9216, 9216, (3, 1, 2), [(1, 1, 2, 0), (3, 1, 1, 1)], {}, "pv8", 4e-3),
]


@pytest.mark.parametrize("cid,lq,lk,large,smalls,kn,kind,tol", ATTN_A, ids=[c[0] for c in ATTN_A])
def test_attention_sample_does_not_depend_on_its_launch(dev, cid, lq, lk, large, smalls, kn, kind, tol, knobs):
    """Table A: the samples / heads a small launch shares with the large one are bit-equal (head h of the H-head launch = the one-head
    launch on the view that starts 64 h elements later); the large launch with (nb0, sb0) and (nb1, sb1) exchanged gives the same
    bits (the b0 / b1 decode); two launches of one input are equal; the first small launch against fp64."""
    knobs(**kn)
    pv8 = kind.startswith("pv8")
    P = _Attn(dev, *large, lq, lk, seed=3, prescaled=kind != "plain")
    ws = _split_ws(P, *large, dev) if kind.endswith("ws") else None  # sized for the large launch in every launch
    big = P.run(*large, ws=ws, pv8=pv8)
    assert _same(big, P.run(*large, ws=ws, pv8=pv8)), f"{cid}: two launches of the same input differ"
    assert _same(big, P.run(*large, swap=True, ws=ws, pv8=pv8)), f"{cid}: (nb0, nb1) = {large[:2]} and exchanged differ"
    for i, cfg in enumerate(smalls):
        out = P.run(*cfg, ws=ws, pv8=pv8)
        assert _same(P.oview(out, *cfg), P.oview(big, *cfg)), f"{cid}: launch (nb0, nb1, H, head0) = {cfg} differs from {large}"
        if i == 0:
            err = _attn_error(P, out, cfg, pv8)
            print(f"\n[attention A] {cid}: launch {cfg} vs fp64 rel-L2 {err:.3e} (bound {tol:g})", flush=True)
            assert err < tol, err
        del out


# id, (nb0, nb1, H), [(lq, lk) for pitch pad 8, (lq, lk) for pad 72], knobs, kind, bound; lk % 64 in {1, 33, 63}, lq % 256 in
# {1, 255} on the 256-row kernels, lq % 128 != 0 on the 4-wave kernel, lq != lk, 3 rows between samples
ATTN_B = [
    ("temporal_1wave", (2, 50, 2), [(21, 33), (24, 63)], {}, "pre", 2e-3),
    ("cross_plain_scale", (2, 1, 3), [(1301, 33), (333, 1)], {}, "plain", 2e-3),
    ("frame_4wave", (3, 1, 2), [(333, 319), (130, 65)], {}, "pre", 2e-3),
    ("frame_attn16", (2, 1, 2), [(2049, 2111), (2303, 2081)], {}, "pre", 1e-3),
    ("frame_attn2", (2, 1, 2), [(767, 1281), (513, 1313)], {"attn_two": 1}, "pre", 1e-3),
    ("joint_split", (2, 1, 2), [(2303, 6177), (2049, 6207)], {}, "ws", 1e-3),
    ("joint_split_forced", (2, 1, 2), [(2049, 1313), (2303, 1343)], {"attn_split": 3}, "ws", 1e-3),
    ("pv8", (2, 1, 2), [(2303, 2111), (2049, 2081)], {}, "pv8", 4e-3),
    ("pv8_split", (2, 1, 2), [(2049, 6145), (2303, 6177)], {}, "pv8ws", 4e-3),
    # >= 6144 keys and no workspace: the unsplit kernels over ragged key counts (what the per-frame regime launches)
    ("frame_attn16_unsplit", (2, 1, 2), [(2303, 6913), (2049, 9215)], {}, "pre", 1e-3),
    ("pv8_unsplit_no_ws", (2, 1, 2), [(2049, 6945), (2303, 9215)], {}, "pv8", 4e-3),
]


@pytest.mark.parametrize("pad", [8, 72], ids=["pad8", "pad72"])
@pytest.mark.parametrize("cid,batch,shapes,kn,kind,tol", ATTN_B, ids=[c[0] for c in ATTN_B])
def test_attention_strides_guards_and_poison(dev, cid, batch, shapes, kn, kind, tol, pad, knobs):
    """Table B: padded pitches, a gap between samples, ragged last key tile and query block; NaN guards around `out`; NaN in every
    place the kernel may address but must not use (q rows >= lq, k / v rows >= lk -- for pv8 the rows the quantiser zero-pads --,
    pitch gaps, the split workspace) changes no bit against zeros there; fp64."""
    knobs(**kn)
    pv8 = kind.startswith("pv8")
    lq, lk = shapes[0 if pad == 8 else 1]
    outs = []
    for poison in (NAN, 0.0):
        P = _Attn(dev, *batch, lq, lk, pad=pad, gap=3, seed=5, poison=poison, prescaled=kind != "plain")
        ws = _split_ws(P, *batch, dev) if kind.endswith("ws") else None
        outs.append(P.run(*batch, ws=ws, pv8=pv8))
    assert _same(outs[0], outs[1]), f"{cid}: NaN behind the logical operands changes the result"
    err = _attn_error(P, outs[0], (*batch, 0), pv8)
    print(f"\n[attention B] {cid} pad {pad} lq {lq} lk {lk}: vs fp64 rel-L2 {err:.3e} (bound {tol:g})", flush=True)
    assert err < tol, err


@pytest.mark.parametrize("what", ["stride_not_multiple_of_8", "pointer_off_16_bytes", "split_workspace_one_float_short"])
def test_attention_argument_checks_are_loud(dev, what, knobs):
    """Each existing argument check raises SevaNativeError and leaves the guarded output untouched."""
    from seva import ops
    from seva._native import SevaNativeError
    knobs(attn_split=3)
    B, H, lq, lk = 2, 2, 2049, 1313
    P = _Attn(dev, B, 1, H, lq, lk, pad=8, gap=3, seed=7)
    out = torch.full_like(P.q, NAN)
    need = ops.attention_split_workspace_numel(B, H, lq, 3)
    ws = torch.full((need,), NAN, device=dev)
    q, qs = P.q, P.qs
    if what == "stride_not_multiple_of_8":
        qs = (qs[0], qs[1], qs[2] + 4)
    elif what == "pointer_off_16_bytes":
        q = P.q[4:]
    else:
        ws = ws[:need - 1]
    with pytest.raises(SevaNativeError):
        ops.attention(q, P.k, P.v, out, nb0=B, nb1=1, heads=H, lq=lq, lk=lk, q_strides=qs, k_strides=P.ks, o_strides=P.os,
                      q_prescaled=True, split_ws=ws)
    torch.cuda.synchronize()
    assert _outside_untouched(out), f"{what}: the refused launch wrote to the output"
    # the same call with the arguments put right is accepted (the check above tested the argument, not something else)
    ops.attention(P.q, P.k, P.v, out, nb0=B, nb1=1, heads=H, lq=lq, lk=lk, q_strides=P.qs, k_strides=P.ks, o_strides=P.os,
                  q_prescaled=True, split_ws=torch.full((need,), NAN, device=dev))
    torch.cuda.synchronize()
    assert torch.isfinite(P.oview(out, B, 1, H)).all()


class _SmallAttn:
    """attn_small_kernel operands: [B][L + gap][pitch] f16 buffers + 256 rows of room, pitch = H * D + pad; poison elsewhere"""

    def __init__(self, dev, B, H, L, D, *, pad=0, gap=0, seed=1, poison=NAN):
        self.dev, self.B, self.H, self.L, self.D = dev, B, H, L, D
        P = self.pitch = H * D + pad
        self.st = ((L + gap) * P, P)

        def buf(sd):
            b = torch.full((B * self.st[0] + 256 * P,), poison, dtype=F16, device=dev)
            data = _randn((B, L, H * D), dev, sd).half()
            torch.as_strided(b, data.shape, (self.st[0], P, 1)).copy_(data)
            return b

        self.q, self.k, self.v = buf(seed), buf(seed + 1), buf(seed + 2)

    def view(self, b, B):  # [B, H, L, D]
        return torch.as_strided(b, (B, self.H, self.L, self.D), (self.st[0], self.D, self.st[1], 1))

    def run(self, B):
        from seva import ops
        out = torch.full_like(self.q, NAN)
        ops.attention_small(self.q, self.k, self.v, out, batch=B, heads=self.H, L=self.L, head_dim=self.D, q_strides=self.st,
                            k_strides=self.st, o_strides=self.st, scale=self.D ** -0.5)
        torch.cuda.synchronize()
        o = self.view(out, B)
        assert torch.isfinite(o).all() and _outside_untouched(out, o)
        return out

    def ref(self, B):
        q, k, v = (self.view(t, B).double() for t in (self.q, self.k, self.v))
        return torch.softmax(q @ k.transpose(-1, -2) * self.D ** -0.5, -1) @ v


@pytest.mark.parametrize("pad", [0, 8, 72], ids=["small-batch1_vs_21", "small-pad8", "small-pad72"])
def test_attention_small_batch_strides_and_poison(dev, pad):
    """CLIP's attention (L = 257, D = 80, 16 heads).  pad 0: batch 1 (qchunks 8) against batch 21 (qchunks 1), bitwise, and fp64.
    pad 8 / 72: padded pitch, 3 rows between samples, NaN there against zeros, guards, fp64 (bound of test_clip_gpu.py: 1e-3)."""
    if pad == 0:
        P = _SmallAttn(dev, 21, 16, 257, 80, seed=9)
        big, one = P.run(21), P.run(1)
        assert _same(big, P.run(21)), "two launches differ"
        assert _same(P.view(one, 1), P.view(big, 1)), "sample 0 of batch 1 differs from sample 0 of batch 21"
        err = rel_l2(P.view(one, 1), P.ref(1))
    else:
        outs = []
        for poison in (NAN, 0.0):
            P = _SmallAttn(dev, 3, 16, 257, 80, pad=pad, gap=3, seed=9, poison=poison)
            outs.append(P.run(3))
        assert _same(outs[0], outs[1]), "NaN behind the logical operands changes the result"
        err = rel_l2(P.view(outs[0], 3), P.ref(3))
    print(f"\n[attention small] pad {pad}: vs fp64 rel-L2 {err:.3e} (bound 1e-3)", flush=True)
    assert err < 1e-3


# ------------------------------------------------------------------------------------------------------------------------------
# C. LayerNorm across the LN_ROWS switch
# ------------------------------------------------------------------------------------------------------------------------------
LN_OUT = {"f16": F16, "e4m3": U8, "f32": F32}


@pytest.mark.parametrize("kind", list(LN_OUT))
@pytest.mark.parametrize("c", [64, 320, 640, 1280], ids=lambda c: f"layernorm_c{c}")
def test_layernorm_rows_do_not_depend_on_the_row_count(dev, c, kind):
    """Rows [0, m) of a launch below 65536 rows (one row per 16-lane group) are bitwise the rows of a launch at or above it (four rows
    per group) on the same leading data: the project's own pair 41 472 / 82 944 at C = 320 (one rank of the CFG split / the full
    batch at T = 8, 576 x 576), 1000 / 65536 + 37 elsewhere (a last block whose groups run past `rows`: the clamped duplicate load
    and the skipped store).  NaN rows behind the input, NaN / 0x7F guard rows behind the output and, for e4m3 at C = 320, in the
    pad bytes of the 384-byte row pitch.  The large launch against fp64."""
    from seva import ops
    m, rows = (41472, 82944) if c == 320 else (1000, 65536 + 37)
    dt = LN_OUT[kind]
    ld = 384 if (kind == "e4m3" and c == 320) else c
    xbuf = torch.full((rows + 256, c), NAN, device=dev)
    xbuf[:rows] = _randn((rows, c), dev, 1) * 3 + 1
    g, b = 1 + 0.1 * _randn((c,), dev, 2), 0.1 * _randn((c,), dev, 3)

    def run(r):
        buf = _guarded((r + 16, ld), dt, dev)
        ops.layernorm(xbuf[:r], g, b, buf[:r])
        torch.cuda.synchronize()
        assert _outside_untouched(buf, buf[:r, :c]), f"rows = {r}: written outside [rows) x [c)"
        return buf[:r, :c]

    small, large = run(m), run(rows)
    assert _same(large, run(rows)), "two launches differ"
    diff = (_bits(small) != _bits(large[:m])).any(1)
    assert not bool(diff.any()), (f"C = {c} {kind}: {int(diff.sum())} of the first {m} rows differ between rows = {m} and rows = {rows}; "
                                  f"first at row {int(diff.nonzero()[0])}")
    ref = F.layer_norm(xbuf[:rows].double(), (c,), g.double(), b.double(), 1e-5)
    if kind == "f16":
        err, mx = rel_l2(large, ref), float((large.double() - ref).abs().max())
        print(f"\n[layernorm] C = {c} f16 rows = {rows}: vs fp64 rel-L2 {err:.3e} (bound 6e-4), max abs {mx:.3e} (bound 4e-3)", flush=True)
        assert err < 6e-4 and mx < 4e-3
    elif kind == "e4m3":
        same = _close_fp8(large.contiguous(), ref.float())
        print(f"\n[layernorm] C = {c} e4m3 rows = {rows}: {same * 100:.3f} % identical to the e4m3 cast of the fp64 result", flush=True)
    else:
        t32 = F.layer_norm(xbuf[:rows].cpu(), (c,), g.cpu(), b.cpu(), 1e-5)
        e_torch = rel_l2(t32, ref.cpu())
        err = rel_l2(large, ref)
        print(f"\n[layernorm] C = {c} fp32 rows = {rows}: vs fp64 rel-L2 {err:.3e}; torch's fp32 layer_norm on the CPU {e_torch:.3e} "
              f"(bound 4x = {4 * e_torch:.3e})", flush=True)
        assert torch.isfinite(large).all() and err < 4 * e_torch


# ------------------------------------------------------------------------------------------------------------------------------
# C. GroupNorm statistics pass across its partitions
# ------------------------------------------------------------------------------------------------------------------------------
GN = [  # id, hw, c1, c2, n of the large launch, SiLU, modulation components, extra output
    ("unet_5184_c320_mod_silu_outf8", 5184, 320, 0, 42, True, 6, "f8"),
    ("unet_1296_c640+320_mod_splitraw", 1296, 640, 320, 42, True, 6, "split_raw"),
    ("unet_324_c1280+640_480quads_512threads", 324, 1280, 640, 42, True, 6, None),
    ("unet_81_c1280+1280_3zchunks_splitout", 81, 1280, 1280, 42, True, 0, "split_out"),
    ("unet_81_c64_dense4_pixels_per_block", 81, 64, 0, 42, False, 4, None),
    ("unet_37_c640+320_fewer_pixels_than_lanes", 37, 640, 320, 42, True, 6, None),
    ("vae_144x144_c512", 20736, 512, 0, 2, True, 0, None),
    ("vae_288x288_c256", 82944, 256, 0, 2, True, 0, None),
    ("vae_576x576_c128", 331776, 128, 0, 2, True, 0, None),
]


def _gn_ref(x, gamma, beta, eps, silu, dmap, dw, db):
    """fp64 GroupNorm(32) (+ SiLU, + modulation) of one sample x [hw, C]"""
    hw, C = x.shape
    xg = x.double().view(hw, 32, C // 32)
    mean, var = xg.mean((0, 2), keepdim=True), xg.var((0, 2), unbiased=False, keepdim=True)
    y = ((xg - mean) / torch.sqrt(var + eps)).view(hw, C) * gamma.double() + beta.double()
    if silu:
        y = y * torch.sigmoid(y)
    if dmap is not None:
        d = dmap.double() @ dw.double().T + db.double()
        y = y * (1 + d[:, :C]) + d[:, C:]
    return y


@pytest.mark.parametrize("cid,hw,c1,c2,n_large,silu,dc,extra", GN, ids=["groupnorm-" + c[0] for c in GN])
def test_groupnorm_sample_does_not_depend_on_the_batch(dev, cid, hw, c1, c2, n_large, silu, dc, extra, knobs):
    """stats1 = None (the separate statistics pass): sample 0 alone is bitwise sample 0 of the batch in every output (out_f16,
    raw_f16 and the case's extra one), with the apply partition moved by the gn_min_iter knob (4, 96) too; one extra NaN sample behind
    every output and the pad bytes of out_f8 stay untouched; sample 0 against fp64 with the bounds of test_groupnorm."""
    from seva import ops
    C = c1 + c2
    x1 = _randn((n_large, hw, c1), dev, 1) * 2 + 0.5
    x2 = _randn((n_large, hw, c2), dev, 2) - 1.0 if c2 else None
    gamma, beta = 1 + 0.1 * _randn((C,), dev, 3), 0.1 * _randn((C,), dev, 4)
    dmap = _randn((n_large, hw, dc), dev, 5) if dc else None
    dw = _randn((2 * C, dc), dev, 6, 0.3) if dc else None
    db = _randn((2 * C,), dev, 7, 0.1) if dc else None
    eps = 1e-5 if silu else 1e-6
    ld8 = C + 64

    def run(n, min_iter=-1):
        knobs(gn_min_iter=min_iter)
        bufs = {"out": _guarded((n + 1, hw, 2 * C if extra == "split_out" else C), F16, dev),
                "raw": _guarded((n + 1, hw, 2 * C if extra == "split_raw" else C), F16, dev)}
        if extra == "f8":
            bufs["f8"] = _guarded((n + 1, hw, ld8), U8, dev)
        ops.groupnorm(x1[:n], x2[:n] if c2 else None, gamma, beta, bufs["out"][:n], ops.groupnorm_workspace(n, dev), eps=eps, silu=silu,
                      dense=dmap[:n] if dc else None, dense_w=dw, dense_b=db, raw_f16=bufs["raw"][:n],
                      out_f8=bufs["f8"][:n] if extra == "f8" else None, split_out=extra == "split_out", split_raw=extra == "split_raw")
        torch.cuda.synchronize()
        res = {}
        for k, buf in bufs.items():
            res[k] = buf[:n, :, :C] if k == "f8" else buf[:n]
            assert _outside_untouched(buf, res[k]), f"{cid}: output {k} (n = {n}): written outside the logical output"
        return res

    one, many = run(1), run(n_large)
    for k in one:
        assert _same(one[k][0], many[k][0]), f"{cid}: output {k} of sample 0 differs between n = 1 and n = {n_large}"
    for mi in (4, 96):
        moved = run(n_large, mi)
        for k in many:
            assert _same(moved[k], many[k]), f"{cid}: output {k} changes with gn_min_iter = {mi}"
        del moved
    del many
    x = torch.cat([x1[0], x2[0]], -1) if c2 else x1[0]
    ref = _gn_ref(x, gamma, beta, eps, silu, dmap[0] if dc else None, dw, db)
    got = one["out"][0, :, :C]
    err, mx = rel_l2(got, ref), float((got.double() - ref).abs().max() / ref.abs().max())
    print(f"\n[groupnorm] {cid}: sample 0 vs fp64 rel-L2 {err:.3e} (bound 6e-4), max abs / max|ref| {mx:.3e} (bound 2e-3)", flush=True)
    assert torch.isfinite(got).all() and err < 6e-4 and mx < 2e-3
    assert _same(one["raw"][0, :, :C], x.half()), "raw_f16 is not the f16 cast of the input"
    if extra == "split_raw":
        assert _same(one["raw"][0, :, C:], (x - x.half().float()).half()), "low half of raw_f16"
    if extra == "split_out":  # [hi | lo]: the sum carries the fp32 result beyond f16's 11 bits
        assert rel_l2(got.double() + one["out"][0, :, C:].double(), ref) < 0.1 * err
    if extra == "f8":
        _close_fp8(one["f8"][0].contiguous(), ref.float())


# ------------------------------------------------------------------------------------------------------------------------------
# C. softmax_rows at the VAE mid block's size
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols,cols_pad", [(5184, 5184), (5183, 5248), (6912, 6912), (6911, 6976)],
                         ids=["softmax_rows-5184", "softmax_rows-5183_pad5248", "softmax_rows-6912", "softmax_rows-6911_pad6976"])
@pytest.mark.parametrize("data", ["random", "dominant_column"])
def test_softmax_rows_at_the_vae_size(dev, cols, cols_pad, data):
    """rows = 5184 (72x72 latent; 6912 for the 72x96 / 96x72 latent's columns), scale 512^-0.5, ldx / ldo larger than needed with
    NaN in the input gap and guards in the output gap and behind the last row; pad columns exactly +0; against an fp64 softmax
    (max abs 1e-3); row 0 and the last row launched alone are bitwise the rows of the full launch.  dominant_column: one column per
    row beats the rest by more than 200 after scaling, in the first, a middle and the last 256-column stride of the kernel's loops."""
    from seva import ops
    rows, scale = (5184 if cols <= 5184 else 6912), 512 ** -0.5
    ldx, ldo = cols + 24, cols_pad + 40
    xbuf = torch.full((rows + 1, ldx), NAN, device=dev)
    x = _randn((rows, cols), dev, 11, 30.0)
    if data == "dominant_column":
        at = torch.tensor([3, 256 * 9 + 77, cols - 1], device=dev)[torch.arange(rows, device=dev) % 3]
        x[torch.arange(rows, device=dev), at] = 8000.0  # 353 after scaling; the rest stays within +- 8
    xbuf[:rows, :cols] = x

    def run(r0, r1):
        buf = _guarded((r1 - r0 + 1, ldo), F16, dev)
        ops.softmax_rows(xbuf[r0:r1], buf[:r1 - r0, :cols_pad], cols, scale)
        torch.cuda.synchronize()
        assert _outside_untouched(buf, buf[:r1 - r0, :cols_pad]), "written outside [rows) x [cols_pad)"
        return buf[:r1 - r0, :cols_pad]

    full = run(0, rows)
    assert torch.isfinite(full).all()
    assert bool((_bits(full[:, cols:]) == 0).all()), "pad columns are not +0"
    for r in (0, rows - 1):
        assert _same(run(r, r + 1)[0], full[r]), f"row {r} alone differs from row {r} of {rows}"
    ref = torch.softmax(x.double() * scale, -1)
    mx = float((full[:, :cols].double() - ref).abs().max())
    print(f"\n[softmax_rows] cols {cols} pad {cols_pad} {data}: max abs vs fp64 {mx:.3e} (bound 1e-3)", flush=True)
    assert mx < 1e-3


# ------------------------------------------------------------------------------------------------------------------------------
# D. elementwise and layout kernels beyond the grid cap
# ------------------------------------------------------------------------------------------------------------------------------
GRID_CAP_ITEMS = 8192 * 256  # csrc/elementwise.hip grid_for: above this many work items the grid-stride loop runs


def _per_row(n, lo, hi, dev, mul=37):
    """n distinct values in [lo, hi) in a scrambled order (a wrong row decode picks a different one)"""
    return lo + (hi - lo) * ((torch.arange(n, device=dev) * mul) % n).float() / n


def _col(s):
    return s.double()[:, None, None, None]


def _ew_case(op, big, dev):
    """-> (inputs: dict of tensors whose leading dim is n (2 n for den2), call(inputs, out), shape of an output of k rows, out dtype,
    ref(inputs) in fp64 (or the fp32 expression the ABI states), comparison, work items of the launch)"""
    from seva import ops
    n, c, h, w = (168, 4, 72, 72) if big else (3, 5, 1, 1)  # the 168-view trajectory's latents; odd: chw = 5, hw = 1
    lat = lambda seed, scale=1.0, lead=n, ch=c: _randn((lead, ch, h, w), dev, seed, scale)  # noqa: E731
    items = n * c * h * w
    shape = lambda k: (k, c, h, w)  # noqa: E731
    close = ("close", 1e-6, 1e-6)  # rtol = atol of test_sampler_elementwise (the chains are built with -ffp-contract=fast)
    if op == "replace_blend":
        rep = lat(2, ch=c + 1)
        rep[:, c] = (torch.arange(n, device=dev) % 2).float()[:, None, None]
        i = dict(x=lat(1, 10.0), rep=rep)
        ref = lambda i: i["x"].double() * (1 - i["rep"][:, c:].double()) + i["rep"][:, :c].double() * i["rep"][:, c:].double()  # noqa: E731
        return i, lambda i, o: ops.replace_blend(i["x"], i["rep"], o), shape, F32, ref, "exact", items
    if op == "denoiser_combine":
        # c_skip = 1 (the discrete denoiser's) keeps x * c_skip exact and |c_out| <= 2.5 keeps |net * c_out| < 16: whichever product the
        # compiler folds into the FMA, the other one's rounding stays below 2^-24 * 16 < 1e-6 where the sum cancels
        i = dict(net=lat(3), x=lat(1, 10.0), co=-_per_row(n, 0.5, 2.5, dev), cs=torch.ones(n, device=dev))
        ref = lambda i: i["net"].double() * _col(i["co"]) + i["x"].double() * _col(i["cs"])  # noqa: E731
        return i, lambda i, o: ops.denoiser_combine(i["net"], i["x"], i["co"], i["cs"], o), shape, F32, ref, close, items
    if op == "add_noise":
        i = dict(x=lat(1, 10.0), eps=lat(4), ns=_per_row(n, 0.05, 1.0, dev))
        ref = lambda i: i["x"].double() + i["eps"].double() * _col(i["ns"])  # noqa: E731
        return i, lambda i, o: ops.add_noise(i["x"], i["eps"], i["ns"], o), shape, F32, ref, close, items
    # Euler chains: r = |dt / sigma| <= 0.57.  Where x + dt (x - den) / sigma cancels, |x - den| = |x| / r with |x| <= |den| r / (1 - r),
    # so the rounding of the difference, 2^-24 |x - den| r, stays below the absolute tolerance; elsewhere the result is of x's size
    sh, dt = _per_row(n, 3.0, 6.0, dev), -_per_row(n, 0.5, 1.7, dev, mul=55)
    if op == "cfg_euler":
        i = dict(x=lat(1, 10.0), den2=lat(5, lead=2 * n), scale=_per_row(n, 1.2, 2.0, dev, mul=11), sh=sh, dt=dt)

        def ref(i):
            k = i["x"].shape[0]
            u, cnd = i["den2"][:k].double(), i["den2"][k:].double()
            den = u + _col(i["scale"]) * (cnd - u)
            return i["x"].double() + _col(i["dt"]) * ((i["x"].double() - den) / _col(i["sh"]))

        return (i, lambda i, o: ops.cfg_euler(i["x"], i["den2"], i["scale"], i["sh"], i["dt"], o), shape, F32, ref,
                ("close", 1e-5, 1e-5), items)
    if op == "cfg_combine":
        i = dict(den2=lat(5, lead=2 * n), scale=_per_row(n, 1.2, 2.0, dev, mul=11))

        def ref(i):
            k = i["scale"].shape[0]
            u, cnd = i["den2"][:k].double(), i["den2"][k:].double()
            return u + _col(i["scale"]) * (cnd - u)

        return i, lambda i, o: ops.cfg_combine(i["den2"], i["scale"], o), shape, F32, ref, close, items
    if op == "euler_step":
        i = dict(x=lat(1, 10.0), den=lat(6), sh=sh, dt=dt)
        ref = lambda i: i["x"].double() + _col(i["dt"]) * ((i["x"].double() - i["den"].double()) / _col(i["sh"]))  # noqa: E731
        return i, lambda i, o: ops.euler_step(i["x"], i["den"], i["sh"], i["dt"], o), shape, F32, ref, close, items
    if op == "to_d":
        i = dict(x=lat(1, 10.0), den=lat(6), sigma=sh)
        ref = lambda i: (i["x"].double() - i["den"].double()) / _col(i["sigma"])  # noqa: E731
        return i, lambda i, o: ops.to_d(i["x"], i["den"], i["sigma"], o), shape, F32, ref, close, items
    if op == "scale_rows":  # one multiplication: rounded once, exact
        i = dict(x=lat(1, 10.0), s=_per_row(n, 0.01, 1.0, dev))
        return i, lambda i, o: ops.scale_rows(i["x"], i["s"], o), shape, F32, lambda i: i["x"].double() * _col(i["s"]), "exact", items
    if op == "add_f32":  # one work item per 4 floats: three trajectories' worth of latents to pass the cap; one addition: exact
        m = 3 * n if big else 1
        ch = c if big else 4
        i = dict(a=lat(7, lead=m, ch=ch), b=lat(8, 3.0, lead=m, ch=ch))
        return (i, lambda i, o: ops.add_f32(i["a"], i["b"], o), lambda k: (k, ch, h, w), F32, lambda i: i["a"].double() + i["b"].double(),
                "exact", m * ch * h * w // 4)
    if op == "silu_f16":  # bound of test_layout_and_elementwise on its distribution (randn)
        i = dict(x=lat(9))
        return (i, lambda i, o: ops.silu_f16(i["x"], o), shape, F16, lambda i: i["x"].double() * torch.sigmoid(i["x"].double()),
                ("abs", 2e-3), items)
    if op == "cast_concat_f16":
        rows, c1, c2 = (217728, 320, 320) if big else (3, 4, 0)  # 42 frames x 5184 tokens; odd: one quad per row, no second source
        i = dict(x1=_randn((rows, c1), dev, 1, 5.0))
        if c2:
            i["x2"] = _randn((rows, c2), dev, 2, 5.0)
        ref = lambda i: torch.cat([i["x1"], i["x2"]], 1) if c2 else i["x1"]  # noqa: E731
        return (i, lambda i, o: ops.cast_concat_f16(i["x1"], i.get("x2"), o), lambda k: (k, c1 + c2), F16, ref, "exact",
                rows * (c1 + c2) // 4)
    if op in ("nchw_to_nhwc_f16", "nchw_to_nhwc_f16_split"):
        # the VAE encoder's 7 frames of 576 x 576 at the stem's 4 + 7 -> 64 channels; odd: one image of one pixel, 3 + 2 channels
        split = op.endswith("split")
        k, c1, c2, hh, cpad = (7, 4, 7, 576, 64) if big else (1, 3, 2, 1, 16)
        i = dict(x1=_randn((k, c1, hh, hh), dev, 1, 30.0), x2=_randn((k, c2, hh, hh), dev, 2), sc=_per_row(k, 0.5, 1.5, dev))

        def ref(i):  # the ABI's expression: the per-image scale is an fp32 multiplication, then one cast (lo: of the fp32 remainder)
            kk = i["x1"].shape[0]
            v = torch.cat([i["x1"] * i["sc"][:, None, None, None], i["x2"]], 1).permute(0, 2, 3, 1).reshape(kk, hh * hh, c1 + c2)
            hi = v.half()
            parts = [hi, (v - hi.float()).half()] if split else [hi]
            parts.append(torch.zeros((kk, hh * hh, cpad - sum(p.shape[-1] for p in parts)), dtype=F16, device=dev))
            return torch.cat(parts, -1)

        return (i, lambda i, o: ops.nchw_to_nhwc_f16(i["x1"], i["x2"], o, scale=i["sc"], split=split), lambda kk: (kk, hh * hh, cpad), F16,
                ref, "exact", k * hh * hh)
    if op == "nhwc_to_nchw_f32":  # the VAE decoder's 7 x 3 x 576 x 576 output from a wider channels-last tensor
        k, ch, hh, ld = (7, 3, 576, 8) if big else (1, 3, 1, 5)
        i = dict(x=_randn((k, hh * hh, ld), dev, 1))
        ref = lambda i: i["x"][..., :ch].reshape(-1, hh, hh, ch).permute(0, 3, 1, 2)  # noqa: E731
        return i, lambda i, o: ops.nhwc_to_nchw_f32(i["x"], o), lambda kk: (kk, ch, hh, hh), F32, ref, "exact", k * ch * hh * hh
    if op == "bilinear_to_nhwc":  # the Pluecker maps to 576 x 576 for two frames; odd: 3 x 5 -> 7 x 1 (ow = 1: rx = 0)
        k, ch, sh_, sw_, oh, ow = (2, 6, 72, 72, 576, 576) if big else (1, 3, 3, 5, 7, 1)
        i = dict(src=_randn((k, ch, sh_, sw_), dev, 1))
        # the comparison test_layout_and_elementwise makes: allclose(atol = 2e-6) with its default rtol = 1e-5
        return (i, lambda i, o: ops.bilinear_to_nhwc(i["src"], o, oh, ow), lambda kk: (kk, oh * ow, ch), F32,
                lambda i: _bilinear_ref(i["src"], oh, ow), ("close", 1e-5, 2e-6), k * oh * ow * ch)
    raise KeyError(op)


def _bilinear_ref(src, oh, ow):
    """F.interpolate(bilinear, align_corners=True) as the ABI states it: the source coordinate dst * (in - 1) / (out - 1) is an fp32
    quantity (ratio and product rounded to fp32, as ATen and the kernel compute it); the four-point blend in fp64.
    -> (result [n, oh * ow, c], slack).  The coordinate f = ratio * dst is only defined to half an ulp of fp32: the kernel takes the
    integer part from the rounded product, and -ffp-contract=fast lets the compiler form the weight f - floor(f) from the unrounded
    one (an FMA; what hipcc emits today).  Both are the ABI's expression, so the comparison allows, on top of the bound
    test_layout_and_elementwise uses, that uncertainty times the slope of the blend: 2^-24 (fy |bottom - top| + fx |right - left|),
    at most ~3e-5 at 72 -> 576 and zero wherever the coordinate is exact.  A wrong decode or weight is an error of the data's size."""
    n, c, sh, sw = src.shape
    dev = src.device

    def axis(s, o):
        r = (torch.tensor(float(s - 1), device=dev) / torch.tensor(float(o - 1), device=dev)) if o > 1 else torch.zeros((), device=dev)
        f = r * torch.arange(o, device=dev, dtype=F32)
        i0 = f.long()
        i1 = i0 + (i0 < s - 1).long()
        return i0, i1, (f - i0.float()).double()

    y0, y1, ly = axis(sh, oh)
    x0, x1, lx = axis(sw, ow)
    s = src.double()
    ly, lx = ly[:, None], lx[None, :]
    top = (1 - lx) * s[:, :, y0][:, :, :, x0] + lx * s[:, :, y0][:, :, :, x1]
    bot = (1 - lx) * s[:, :, y1][:, :, :, x0] + lx * s[:, :, y1][:, :, :, x1]
    # slack: half an ulp of each coordinate (<= 2^-24 f) times the slope of the blend along it
    fy, fx = (y0.double() + ly[:, 0])[:, None], (x0.double() + lx[0])[None, :]
    dx = (1 - ly) * (s[:, :, y0][:, :, :, x1] - s[:, :, y0][:, :, :, x0]) + ly * (s[:, :, y1][:, :, :, x1] - s[:, :, y1][:, :, :, x0])
    slack = 2.0 ** -24 * (fy * (bot - top).abs() + fx * dx.abs())
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(n, oh * ow, c)  # noqa: E731
    return nhwc((1 - ly) * top + ly * bot), nhwc(slack)


def _rows_of(inputs, r):
    """the inputs of row r alone: tensors led by n give row r, den2 (led by 2 n) its two halves' rows"""
    n = min(t.shape[0] for t in inputs.values())
    out = {}
    for k, t in inputs.items():
        out[k] = t[r:r + 1] if t.shape[0] == n else torch.cat([t[r:r + 1], t[n + r:n + r + 1]])
    return out, n


EW_OPS = ["nchw_to_nhwc_f16", "nchw_to_nhwc_f16_split", "nhwc_to_nchw_f32", "cast_concat_f16", "bilinear_to_nhwc", "silu_f16", "add_f32",
          "replace_blend", "denoiser_combine", "add_noise", "cfg_euler", "cfg_combine", "euler_step", "to_d", "scale_rows"]


@pytest.mark.parametrize("size", ["big", "odd"])
@pytest.mark.parametrize("op", EW_OPS)
def test_elementwise_beyond_the_grid_cap(dev, op, size):
    """Every entry point of csrc/elementwise.hip once above 8192 x 256 work items (the grid-stride loop and the 64-bit decodes run) at
    a shape the engines use, once at an odd small size.  Reference: the same expression in fp64 on the GPU rounded once to the output
    type; moves, casts, single operations and replace_blend with a 0 / 1 mask exact, the multiply-add chains with the tolerances of
    test_sampler_elementwise; a guard behind the last output element; a row launched alone is bitwise the row of the large launch."""
    big = size == "big"
    inputs, call, shape, dt, ref, cmp, items = _ew_case(op, big, dev)
    assert (items > GRID_CAP_ITEMS) == big, (op, items)
    _, n = _rows_of(inputs, 0)

    def run(i, k):
        numel = math.prod(shape(k))
        buf = _guarded((numel + 64,), dt, dev)
        out = buf[:numel].view(shape(k))
        call(i, out)
        torch.cuda.synchronize()
        assert _outside_untouched(buf, out), f"{op}: written behind the last output element"
        return out

    got = run(inputs, n)
    want, slack = ref(inputs), 0.0
    if isinstance(want, tuple):  # bilinear: the fp32 coordinate's own uncertainty (_bilinear_ref)
        want, slack = want
    assert got.shape == want.shape and torch.isfinite(got).all()
    if cmp == "exact":
        want = want.to(dt)
        bad = _bits(got) != _bits(want)
        assert not bool(bad.any()), f"{op} {size}: {int(bad.sum())} elements differ; first at flat index {int(bad.flatten().nonzero()[0])}"
    elif cmp[0] == "abs":
        mx = float((got.double() - want).abs().max())
        print(f"\n[elementwise] {op} {size}: max abs vs fp64 {mx:.3e} (bound {cmp[1]:g})", flush=True)
        assert mx < cmp[1]
    else:
        _, rtol, atol = cmp
        err = (got.double() - want).abs()
        excess = float((err / (atol + rtol * want.abs() + slack)).max())
        print(f"\n[elementwise] {op} {size}: max |got - fp64| / (atol + rtol |ref|) = {float((err / (atol + rtol * want.abs())).max()):.3f}"
              f" (rtol {rtol:g}, atol {atol:g}); with the coordinate slack (bilinear only) {excess:.3f}", flush=True)
        assert excess <= 1.0, excess
    for r in sorted({n - 1, n // 3}):
        alone = run(_rows_of(inputs, r)[0], 1)
        assert _same(alone[0], got[r]), f"{op} {size}: row {r} launched alone differs from row {r} of {n}"
