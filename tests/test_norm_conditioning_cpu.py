"""The offset-dominated norm cases (tests/norm_cases.py) without a GPU: the yardstick of every case is usable, and an fp32 model of
csrc/norm.hip's GroupNorm statistics pass shows that sums about a per-group pivot stay inside the yardstick bound at every rung
while E[x^2] - mean^2 on the raw values does not -- so the device assertions of tests/test_norm_conditioning_gpu.py can fail.

The model restates the pass in torch: a block of T threads covers C / 4 quads of channels, T / (C / 4) pixel lanes; lane pl walks the
pixels p_begin + pl, p_begin + pl + lanes, ... of its slab and keeps one running fp32 sum and sum of squares per channel; one thread
per group then adds the lanes' partials in order (lane outermost, channel innermost) in fp32; slabs, the division and the variance are
fp64; mean and rstd are stored as fp32.  Multiply and add round separately here (the device may fuse them: one rounding fewer)."""
import math

import pytest
import torch

import norm_cases as NC


def _seq_sum32(t, dim):
    """sequential fp32 sum along `dim`, one rounding per term"""
    acc = torch.zeros_like(t.select(dim, 0))
    for k in range(t.shape[dim]):
        acc = acc + t.select(dim, k)
    return acc


def _partition(hw, C):
    cq = C // 4
    threads = 256 if cq <= 256 else (1024 if cq >= 1024 else 64 * ((cq + 63) // 64))
    lanes = threads // min(cq, threads)
    cap = min(max(hw // 128, 63), 1023)
    return lanes, min(max(hw // (lanes * 16), 1), cap)


def model_stats(x, shifted: bool):
    """-> (mean, rstd) [n, GROUPS] as fp32, of x [n, hw, C] fp32"""
    n, hw, C = x.shape
    cpg = C // NC.GROUPS
    lanes, nslab = _partition(hw, C)
    pivot = x[:, 0, ::cpg].clone() if shifted else torch.zeros((n, NC.GROUPS))
    s = torch.zeros((n, NC.GROUPS), dtype=torch.float64)
    ss = torch.zeros_like(s)
    for slab in range(nslab):
        p0, p1 = slab * hw // nslab, (slab + 1) * hw // nslab
        steps = (p1 - p0 + lanes - 1) // lanes
        blk = torch.zeros((n, steps * lanes, C))
        d = x[:, p0:p1] - pivot.repeat_interleave(cpg, 1)[:, None, :]
        blk[:, :p1 - p0] = d  # a lane past the slab's end adds nothing (+0 leaves an fp32 sum as it is)
        blk = blk.view(n, steps, lanes, C)
        ls, lq = _seq_sum32(blk, 1), _seq_sum32(blk * blk, 1)                    # [n, lanes, C]: the threads' running sums
        fold = lambda t: _seq_sum32(t.view(n, lanes, NC.GROUPS, cpg).permute(0, 2, 1, 3).reshape(n, NC.GROUPS, lanes * cpg), 2)
        s += fold(ls).double()
        ss += fold(lq).double()
    cnt = float(cpg * hw)
    md = s / cnt
    var = (ss / cnt - md * md).clamp_min(0.0)
    return (pivot.double() + md).float(), (1.0 / torch.sqrt(var + NC.EPS)).float()


def _model_error(x, gamma, beta, ref, shifted):
    mean, rstd = model_stats(x, shifted)
    var = 1.0 / rstd.double() ** 2 - NC.EPS
    return NC.rel_l2(NC.gn_normalise64(x, mean.double(), var, gamma, beta), ref)


@pytest.fixture(scope="module", params=[(s, k) for s in NC.GN_SHAPES[:2] for k in NC.KINDS], ids=lambda p: f"{p[0][0]}-{p[1]}")
def small_case(request):
    (sid, hw, c1, c2), kind = request.param
    C = c1 + c2
    x, _ = NC.gn_input(kind, hw, C)
    gamma, beta = NC.affine(C)
    ref = NC.gn_ref64(x, gamma, beta)
    e_torch = NC.rel_l2(NC.gn_torch32(x, gamma, beta), ref)
    return kind, x, gamma, beta, ref, e_torch, NC.e_fmt_split(ref)


def test_partition_of_the_model_reaches_the_paths_the_shapes_are_named_for():
    assert _partition(81, 64) == (16, 1) and _partition(324, 64) == (16, 1)
    assert _partition(1296, 320)[0] == 3 and _partition(1296, 320)[1] > 1
    assert _partition(324, 1920) == (1, 20) and _partition(37, 960) == (1, 2)
    assert _partition(20736, 128)[1] > 63


def test_inputs_are_offset_dominated():
    for r in NC.RUNGS[1:]:
        x, off = NC.gn_input(f"r{r}", 324, 64)
        xg = x.double().view(NC.N, 324, NC.GROUPS, 2)
        ratio = xg.mean((1, 3)).abs() / xg.std((1, 3))
        assert 0.1 * r < float(ratio.min()) and float(ratio.max()) < 3 * r, (r, ratio.min(), ratio.max())
        assert float(off[0, 0]) != float(off[1, 0])  # per sample
    x, _ = NC.gn_input("const", 81, 64)
    assert bool((x[NC.CONST_SAMPLE, :, -2:] == NC.CONST_VALUE).all()) and not bool((x[0, :, -2:] == NC.CONST_VALUE).any())
    x, _ = NC.gn_input("spread", 81, 320)
    g = x[:, :, 10:20].double()
    assert float(g.mean().abs()) < 8 and 50 < float(g.std()) < 80  # between-channel variance dominates: well conditioned


def test_yardstick_is_finite_and_tight(small_case):
    kind, x, gamma, beta, ref, e_torch, e_fmt = small_case
    b = NC.bound(e_torch, e_fmt)
    print(f"\n[yardstick] {kind}: e_torch {e_torch:.3e} e_fmt {e_fmt:.3e} bound {b:.3e}")
    assert math.isfinite(e_torch) and math.isfinite(e_fmt) and torch.isfinite(ref).all()
    assert b < 1e-3  # at r = 512 too: the device assertions mean something
    assert e_fmt < 4 * 2.0 ** -22  # [hi | lo] carries 22 bits


def test_shifted_sums_stay_inside_the_bound(small_case):
    kind, x, gamma, beta, ref, e_torch, e_fmt = small_case
    err, b = _model_error(x, gamma, beta, ref, True), NC.bound(e_torch, e_fmt)
    print(f"\n[model, sums about a pivot] {kind}: {err:.3e} (bound {b:.3e})")
    assert err < b
    if kind == "const":
        mean, rstd = model_stats(x, True)
        assert float(mean[NC.CONST_SAMPLE, NC.CONST_GROUP]) == NC.CONST_VALUE
        assert float(rstd[NC.CONST_SAMPLE, NC.CONST_GROUP]) == pytest.approx(NC.EPS ** -0.5, rel=1e-6)


def test_unshifted_sums_leave_the_bound(small_case):
    """what the statistics pass computed before it took a pivot: outside the bound from r = 64 (the tests can fail)"""
    kind, x, gamma, beta, ref, e_torch, e_fmt = small_case
    err, b = _model_error(x, gamma, beta, ref, False), NC.bound(e_torch, e_fmt)
    print(f"\n[model, E[x^2] - mean^2] {kind}: {err:.3e} (bound {b:.3e})")
    # ("const" is left out: torch's own fp32 result is poor on the constant group, which widens that case's yardstick; the group is
    # pinned by its own ulp bound on the device)
    if kind in ("r64", "r512", "spread"):
        assert err > b
    elif kind == "r0":
        assert err < b


def test_layernorm_yardstick():
    for kind in NC.KINDS[:4]:
        x = NC.ln_input(kind, 1000, 320)
        gamma, beta = NC.affine(320)
        ref = NC.ln_ref64(x, gamma, beta)
        e_torch = NC.rel_l2(NC.ln_torch32(x, gamma, beta), ref)
        assert math.isfinite(e_torch) and NC.bound(e_torch, NC.e_fmt_split(ref)) < 1e-3
        row_ratio = x.double().mean(1).abs() / x.double().std(1)
        assert NC.rung_of(kind) == 0 or 0.25 * NC.rung_of(kind) < float(row_ratio.median()) < 2.5 * NC.rung_of(kind)
