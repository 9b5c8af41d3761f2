"""Every row of the GEMM / conv instantiation tables (csrc/gemm_plan.h) against an fp64 reference, one launch per case of
tests/kernel_cases.py.  tests/test_kernel_coverage_cpu.py keeps the list closed over the tables; here each case

* runs through `kernel_cases.launch` with outputs and the statistics buffer pre-filled with NaN (e4m3: the NaN byte),
* must have taken the row it names (`ops.last_plan()`),
* is compared with fp64 torch (on the CPU) on the same integer operands: activations -4..4, weights -3..3 (e4m3: times a power-of-two
  row scale 2^-2..2^2), bias / row_add / residual -9..9.  Every product and sum is exact in fp32, so there is NO tolerance: out_f32 equals the
  reference, out_f16 its f16 rounding, out_f8 its saturating round-to-nearest-even e4m3, ch_stats the fp64 block sums (2-D tiles and
  the phase rows: the blocks of an image add up to that image), the split-precision output is [f16(v) | f16(v - f32(f16(v)))] bit
  for bit (operands -20..20 / -15..15 there, so that v exceeds 2048 and the low half is not zero).
  The e4m3 cases that emit statistics take operands -2..2 and row scales 1 and 2 (STATS_E4M3_RANGES), so that the 64-row sums of
  squares are exact in fp32 as well; `_operands` asserts that precondition for every statistics case.

The GEGLU rows are the one exception (`_check_geglu`): h gelu(g) is not an integer.
"""
import zlib

import pytest
import torch
import torch.nn.functional as F

import kernel_cases as kc
from test_ops_gpu import _block_stats

pytestmark = pytest.mark.gpu

F64, F16, U8 = torch.float64, torch.float16, torch.uint8
NAN = float("nan")

# Absolute floor of the GEGLU bound.  How it was obtained (CPU only, nothing from the kernel): for every GEGLU case of kernel_cases.py,
# fp32 torch `h * F.gelu(g)` (erf) on the exact integer accumulators against the fp64 reference of `_operands`; the largest error over
# all elements of all cases is 3.32e-4 (case 'geglu 128x128 e4m3 | tail', where |h gelu(g)| reaches 3220: the fp32 roundings of gelu and
# of the product).  Doubled, as the margin for a different but equally valid fp32 erf, and rounded up: 6.7e-4.  `_check_geglu` re-checks on the CPU, before it looks at
# the kernel's output, that the fp32 reference of its case stays inside the bound with HALF this floor.
GEGLU_FLOOR = 6.7e-4

# (|activation|, |weight|, smallest and largest exponent of the row scale) of the e4m3 cases that emit statistics
STATS_E4M3_RANGES = (2, 2, 0, 1)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from seva import _native
    _native.load()
    return torch.device("cuda:0")


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def _to8(x):
    """saturating round-to-nearest-even e4m3 bytes (the emulation of tests/test_output_rounding_gpu.py: torch's own cast)"""
    return x.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(U8)


def _from8(b):
    return b.view(torch.float8_e4m3fn).to(F64)


def _ulp16(r):
    """one f16 ulp of r (subnormal spacing below 2^-14)"""
    e = torch.frexp(r.abs().clamp_min(2.0 ** -14))[1] - 1
    return torch.exp2((e - 10).to(F64))


def _per_image_stats(c):
    """2-D tiles and the phase rows: a block is 64 pixels of one image, not 64 consecutive rows"""
    return "2-D" in c.row or c.kind == "phases128"


def _largest_block_sum_of_squares(c, v):
    """over the 64-row blocks of the statistics; where the partition is the kernel's own (per-image rows): the 64 largest of an image"""
    M, N = v.shape
    if not _per_image_stats(c):
        return float(_block_stats(v, M, N)[:, 1].max())
    n = c.shape[0]
    return float((v * v).view(n, M // n, N).topk(64, dim=1).values.sum(1).max())


def _operands(c):
    """CPU fp64 operands of a case and its fp64 reference: (t, ref) with t[name] = the tensors kernel_cases.launch takes (inputs only,
    in the kernels' layouts and dtypes) and ref = dict(v = the epilogue value [M, N_out], plus what the GEGLU check needs)"""
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    e4m3, split = c.prec == "e4m3", c.kind == "split_out" and not c.geglu
    M, N, K = kc.problem(c)
    t, ref = {}, {}
    alo, wlo, emin, emax = (20, 15, 0, 0) if split else (4, 3, -2, 2)
    if e4m3 and "ch_stats" in c.ops:
        alo, wlo, emin, emax = STATS_E4M3_RANGES  # smaller values, no fractions: the sums of SQUARES of 64 rows have to be exact in fp32 too
    scale = torch.ones(N, dtype=F64)
    if e4m3:
        e = torch.randint(emin, emax + 1, (N,), generator=g)
        if c.geglu:
            e = e.clamp_max(0)  # gate rows: |g| <= 8; value rows: |h| as in the f16 cases, so that one floor serves every GEGLU row
        assert e.unique().numel() >= 2
        t["w_exp"] = (e + 127).to(U8)
        scale = torch.exp2(e.to(F64))
    op = (lambda x: _to8(x)) if e4m3 else (lambda x: x.to(F16))
    if c.kind in kc.GEMM_KINDS:
        a, w = _ints(g, (M, K), -alo, alo), _ints(g, (N, K), -wlo, wlo)
        if c.geglu:  # rows in groups of 64 = [32 value | 32 gate] (include/seva_hip.h); gate rows: |g| <= 8 through one or two +-1 entries
            gate = torch.arange(N) % 64 >= 32
            nz = 1 if "bias" in c.ops else 2
            wg = torch.zeros((int(gate.sum()), K), dtype=F64)
            cols = torch.stack([torch.randperm(K, generator=g)[:nz] for _ in range(wg.shape[0])])
            wg.scatter_(1, cols, _ints(g, cols.shape, 0, 1) * 2 - 1)
            w[gate] = wg
        t["a"], t["w"] = op(a), op(w)
        acc = a @ (w * scale[:, None]).T
    else:
        n, ih, iw, cin, cout = c.shape
        oh, ow = kc.conv_geometry(c)[:2]
        x, w = _ints(g, (n, cin, ih, iw), -alo, alo), _ints(g, (cout, cin, 3, 3), -wlo, wlo)
        from seva._engine import combine_up_phases, pack_conv3x3
        t["x"] = op(x.permute(0, 2, 3, 1).contiguous())
        if c.kind in ("phases", "phases128"):
            t["w"] = combine_up_phases(w.float())  # the project's own packer: [4, cout, 4 cin] f16 (sums of at most four integers)
        else:
            t["w"] = op(pack_conv3x3(w.float()).to(F64))
        xin = F.interpolate(x, scale_factor=2, mode="nearest") if (c.up or c.kind in ("phases", "phases128")) else x
        ws = w * scale[:, None, None, None]
        y = F.conv2d(F.pad(xin, (0, 1, 0, 1)), ws, stride=c.stride) if c.pad_br else F.conv2d(xin, ws, stride=c.stride, padding=1)
        assert y.shape[-2:] == (oh, ow)
        acc = y.permute(0, 2, 3, 1).reshape(M, N)
        if c.k2:
            a2, w2 = _ints(g, (M, c.k2), -4, 4), _ints(g, (N, c.k2), -3, 3)
            t["a2"], t["w"] = a2.to(F16), torch.cat([t["w"], w2.to(F16)], 1).contiguous()
            acc = acc + a2 @ w2.T
    if "bias" in c.ops:
        t["bias"] = _ints(g, (N,), -9, 9)
        if c.geglu:
            gate = torch.arange(N) % 64 >= 32
            t["bias"][gate] = _ints(g, (int(gate.sum()),), -4, 4)
        acc = acc + t["bias"]
    if "row_add" in c.ops:
        t["row_add"] = _ints(g, ((M + c.rpg - 1) // c.rpg, N), -9, 9)
        acc = acc + t["row_add"].repeat_interleave(c.rpg, 0)[:M]
    if "residual" in c.ops:
        t["residual"] = _ints(g, (M, N), -9, 9)
        acc = acc + t["residual"]
    for k in ("bias", "row_add", "residual"):
        if k in t:
            t[k] = t[k].float()
    assert acc.abs().max() < 2.0 ** 22 and torch.equal(acc * 4, (acc * 4).round())  # exact in fp32 whatever the order of the additions
    if "ch_stats" in c.ops:
        # the statistics are fp32 sums of 64 values / squares in an order of the kernel's choosing: exact iff every partial sum is a
        # multiple of 2^-4 (squares of multiples of 2^-2) below 2^24 * 2^-4.  The 64 largest squares of an image bound every block's sum.
        unit = 1.0 if torch.equal(acc, acc.round()) else 1.0 / 16  # squares of integers, or of multiples of 2^-2
        ref["sq_ratio"] = _largest_block_sum_of_squares(c, acc) / unit / 2.0 ** 24
        assert ref["sq_ratio"] < 1, (c.id, ref["sq_ratio"])
    if c.geglu:
        v = acc.view(M, N // 64, 2, 32)
        h, gt = v[:, :, 0].reshape(M, N // 2), v[:, :, 1].reshape(M, N // 2)
        assert gt.abs().max() <= 8
        ref.update(h=h, g=gt, v=h * (0.5 * gt * (1.0 + torch.erf(gt * 0.5 ** 0.5))))
    else:
        ref["v"] = acc
    return t, ref


def _geglu_bound(v, floor=GEGLU_FLOOR):
    return _ulp16(v) + floor


def geglu_fp32_error(c):
    """largest error of fp32 torch GEGLU against the fp64 reference on the case's integers (how GEGLU_FLOOR was obtained)"""
    _, ref = _operands(c)
    return float((ref["h"].float() * F.gelu(ref["g"].float()) - ref["v"]).abs().max())


def _check_geglu(c, ref, out):
    """GEGLU rows: the accumulators h and g are exact integers (|g| <= 8), the reference is fp64 h gelu(g) with erf, and EVERY element of
    every output may differ from it by at most one f16 ulp of the reference + GEGLU_FLOOR (6.7e-4, see there: the floor covers the
    cancelling negative tail of GELU, where the value is far below what an fp32 erf resolves).  Per element, not a norm: one wrong
    column cannot hide.  e4m3 output: between the e4m3 roundings of the two ends of that interval (the rounding is monotone).
    The split-precision output: hi = f16(v), lo = f16(v - f32(hi)) bit for bit of the fp32 value v the same launch wrote to out_f32;
    without an out_f32, hi + lo is held to the bound."""
    v = ref["v"]
    bound = _geglu_bound(v)
    f32 = (ref["h"].float() * F.gelu(ref["g"].float())).to(F64)
    assert bool(((f32 - v).abs() <= _geglu_bound(v, GEGLU_FLOOR / 2)).all()), "the fp32 reference itself leaves the bound"
    NO = v.shape[1]
    for name in ("out_f32", "out_f16"):
        if name not in out:
            continue
        got = out[name].to(F64)
        if c.kind == "split_out" and name == "out_f16":
            hi, lo = out[name][:, :NO], out[name][:, NO:]
            got = hi.to(F64) + lo.to(F64)
            assert bool((lo != 0).any()), "the low half is identically zero"
            if "out_f32" in out:
                v32 = out["out_f32"]
                assert torch.equal(hi.view(torch.int16), v32.to(F16).view(torch.int16)), "hi != f16(v)"
                assert torch.equal(lo.view(torch.int16), (v32 - hi.float()).to(F16).view(torch.int16)), "lo != f16(v - f32(hi))"
        err = (got - v).abs()
        bad = ~(err <= bound)  # (NaN: bad)
        assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements off, worst {float((err / bound).nan_to_num(1e30).max()):.2f} x the bound"
    if "out_f8" in out:
        got, lo, hi = _from8(out["out_f8"]), _from8(_to8(v - bound)), _from8(_to8(v + bound))
        assert bool(((got >= lo) & (got <= hi)).all()), "out_f8 outside the e4m3 roundings of the bound"


def _check_exact(c, ref, out):
    v = ref["v"]
    M, N = v.shape
    if "out_f32" in out:
        assert torch.equal(out["out_f32"].to(F64), v), f"out_f32: max diff {(out['out_f32'].to(F64) - v).abs().max()}"
    if "out_f16" in out:
        if c.kind == "split_out":
            hi, lo = out["out_f16"][:, :N], out["out_f16"][:, N:]
            want_hi = v.to(F16)
            want_lo = (v.float() - want_hi.float()).to(F16)
            assert bool((want_lo != 0).any()), "the low half is identically zero"
            assert torch.equal(hi.view(torch.int16), want_hi.view(torch.int16)), "hi != f16(v)"
            assert torch.equal(lo.view(torch.int16), want_lo.view(torch.int16)), "lo != f16(v - f32(hi))"
        else:
            assert torch.equal(out["out_f16"].to(F64), v.to(F16).to(F64)), "out_f16 != f16(reference)"
    if "out_f8" in out:
        assert torch.equal(_from8(out["out_f8"]), _from8(_to8(v))), "out_f8 != e4m3(reference)"
    if "ch_stats" in out:
        st = out["ch_stats"].to(F64)
        if _per_image_stats(c):
            n = c.shape[0]
            for k, want in ((0, v), (1, v * v)):
                assert torch.equal(st[:, k].view(n, -1, N).sum(1), want.view(n, -1, N).sum(1)), f"ch_stats[{k}]: per-image sums"
        else:
            assert torch.equal(st, _block_stats(v, M, N)), "ch_stats != fp64 block sums"


@pytest.mark.parametrize("cid", [c.id for c in kc.CASES])
def test_row_exact(dev, cid, knobs):
    from seva import ops
    c = kc.BY_ID[cid]
    t, ref = _operands(c)
    M, N, _ = kc.problem(c)
    NO = N // 2 if c.geglu else N
    t = {k: v.to(dev) for k, v in t.items()}
    if "out_f32" in c.ops:
        t["out_f32"] = torch.full((M, NO), NAN, device=dev)
    if "out_f16" in c.ops:
        t["out_f16"] = torch.full((M, 2 * NO if c.kind == "split_out" else NO), NAN, device=dev, dtype=F16)
    if "out_f8" in c.ops:
        t["out_f8"] = torch.full((M, NO), 0x7F, device=dev, dtype=U8)
    if "ch_stats" in c.ops:
        t["ch_stats"] = torch.full(ops.channel_stats_shape(M, N), NAN, device=dev)
    if "splitk_ws" in c.ops:
        t["splitk_ws"] = ops.splitk_workspace(M, N, dev)
    assert set(t) == set(kc.tensors_needed(c))
    if c.kind in kc.CONV_KINDS:  # [n, pixels, channels]
        n = c.shape[0]
        for k in ("residual", "out_f32", "out_f16", "out_f8"):
            if k in t:
                t[k] = t[k].view(n, M // n, -1)
    knobs(**dict(c.knobs))
    kc.launch(ops, c, t)
    torch.cuda.synchronize()
    assert ops.last_plan() == c.row
    if "splitk_ws" in c.ops:
        assert int(t["splitk_ws"][:ops.SPLITK_FLAGS].view(torch.int32).abs().sum()) == 0  # flags re-armed, no consumer gave up
    out = {k: t[k].reshape(M, -1).cpu() if k != "ch_stats" else t[k].cpu() for k in ("out_f32", "out_f16", "out_f8", "ch_stats") if k in t}
    (_check_geglu if c.geglu else _check_exact)(c, ref, out)
