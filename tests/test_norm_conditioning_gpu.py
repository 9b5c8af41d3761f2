"""GroupNorm and LayerNorm on the device against fp64 across |mean| / std ratios r = 0, 8, 64, 512 (tests/norm_cases.py holds the
inputs, the references and the yardstick; tests/test_norm_conditioning_cpu.py shows on an fp32 model that these assertions can fail).

Every other norm test feeds inputs whose mean is about their standard deviation and reads the f16 output, whose rounding floor hides
a statistics error below ~1e-4.  Here every group (row) is offset-dominated, sign and size of the offset differ per group and per
sample, and the main readout is near-fp32: the [hi | lo] split output (GroupNorm, LayerNorm) or the fp32 output (LayerNorm).

A. GroupNorm with its own statistics pass (gn_stats_kernel sums about a per-(sample, group) pivot, gn_finalize_kernel): near-fp32
   readout inside the yardstick bound at every rung and for the two structures of the r = 64 rung (a group whose channels sit at
   +-64: well conditioned; a group that is exactly 100.0: output = beta to one amplified ulp); the f16 readouts (SiLU, SiLU +
   modulation) inside test_groupnorm's bounds; sample 1 alone bitwise sample 1 of the batch.
B. GroupNorm fed with producer statistics (fp32 64-row block sums of a GEMM epilogue, part of the C ABI): finalize + apply pinned
   against an fp64 evaluation of the SAME fp32 block sums; the block sums against fp64; end to end against true fp64 under the derived
   envelope (1 + r^2) 2^-18 + yardstick, with the f16 readout's figures printed per rung (DESIGN.md quotes them).
C. LayerNorm (two-pass): fp32 and split outputs inside the yardstick bound, f16 inside test_layernorm's bounds; the fused
   feed-forward's LayerNorm prologue against the separately normalised operand at r = 64."""
import pytest
import torch

import norm_cases as NC

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from seva import _native
    _native.load()
    return torch.device("cuda:0")


class Case:
    pass


def _split_sources(x, c1, c2, dev):
    x1 = x[..., :c1].contiguous().to(dev)
    x2 = x[..., c1:].contiguous().to(dev) if c2 else None
    return x1, x2


def _run_gn(case, dev, *, n0=0, n1=None, split_out=False, silu=False, mod=None, stats=None):
    from seva import ops
    n1 = case.n if n1 is None else n1
    n, C = n1 - n0, case.C
    out = torch.full((n, case.hw, 2 * C if split_out else C), NAN, device=dev, dtype=F16)
    kw = {}
    if mod is not None:
        kw = dict(dense=mod[0][n0:n1].contiguous().to(dev), dense_w=mod[1].to(dev), dense_b=mod[2].to(dev))
    if stats is not None:
        kw.update(stats1=stats[0], stats2=stats[1])
    ops.groupnorm(case.x1[n0:n1], case.x2[n0:n1] if case.x2 is not None else None, case.gamma_d, case.beta_d, out,
                  ops.groupnorm_workspace(n, dev), eps=NC.EPS, silu=silu, split_out=split_out, **kw)
    torch.cuda.synchronize()
    return out


def _hi_lo(out, C):
    o = out.cpu()
    return o[..., :C].double() + o[..., C:].double()


def _yardstick(case, torch32):
    case.e_torch = NC.rel_l2(torch32, case.ref)
    case.e_fmt = NC.e_fmt_split(case.ref)
    case.bound = NC.bound(case.e_torch, case.e_fmt)


# ------------------------------------------------------------------------------------------------------------------------------
# A. GroupNorm, own statistics pass
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(s, k) for s in NC.GN_SHAPES for k in NC.KINDS], ids=lambda p: f"{p[0][0]}-{p[1]}")
def gn(request, dev):
    (sid, hw, c1, c2), kind = request.param
    c = Case()
    c.id, c.kind, c.hw, c.c1, c.c2, c.C, c.n = f"{sid}-{kind}", kind, hw, c1, c2, c1 + c2, NC.N
    c.x, _ = NC.gn_input(kind, hw, c.C)
    c.gamma, c.beta = NC.affine(c.C)
    c.ref = NC.gn_ref64(c.x, c.gamma, c.beta)
    _yardstick(c, NC.gn_torch32(c.x, c.gamma, c.beta))
    c.x1, c.x2 = _split_sources(c.x, c1, c2, dev)
    c.gamma_d, c.beta_d = c.gamma.to(dev), c.beta.to(dev)
    return c


def test_groupnorm_near_fp32_readout(dev, gn):
    got = _hi_lo(_run_gn(gn, dev, split_out=True), gn.C)
    err = NC.rel_l2(got, gn.ref)
    print(f"\n[groupnorm own pass] {gn.id}: e_torch {gn.e_torch:.3e} e_fmt {gn.e_fmt:.3e} bound {gn.bound:.3e} measured {err:.3e}", flush=True)
    assert torch.isfinite(got).all() and err < gn.bound
    if gn.kind == "const":
        cpg = gn.C // NC.GROUPS
        sl = slice(NC.CONST_GROUP * cpg, (NC.CONST_GROUP + 1) * cpg)
        dev_ = (got[NC.CONST_SAMPLE, :, sl] - gn.beta[sl].double()).abs().amax(0)
        tol = NC.const_group_tolerance(gn.gamma[sl])
        print(f"[groupnorm own pass] {gn.id}: constant group max |y - beta| / tolerance {float((dev_ / tol).max()):.3f}", flush=True)
        assert bool((dev_ <= tol).all()), (dev_, tol)


def test_groupnorm_f16_readout(dev, gn):
    """the bounds of test_groupnorm, unchanged, at every rung"""
    mods = [None] + ([NC.modulation(gn.n, gn.hw, gn.C)] if gn.C >= 320 else [])
    for mod in mods:
        got = _run_gn(gn, dev, silu=True, mod=mod).cpu().double()
        ref = NC.silu_mod64(gn.ref, True, mod)
        err, mx = NC.rel_l2(got, ref), float((got - ref).abs().max() / ref.abs().max())
        print(f"\n[groupnorm own pass] {gn.id} f16 SiLU{' + modulation' if mod else ''}: rel-L2 {err:.3e} (bound 6e-4), "
              f"max abs / max|ref| {mx:.3e} (bound 2e-3)", flush=True)
        assert torch.isfinite(got).all() and err < 6e-4 and mx < 2e-3


def test_groupnorm_sample_alone_is_bitwise_the_sample_in_the_batch(dev, gn):
    """offsets differ per sample: statistics or a pivot taken from the wrong sample show here"""
    both = _run_gn(gn, dev, split_out=True)
    for s in range(gn.n):
        alone = _run_gn(gn, dev, n0=s, n1=s + 1, split_out=True)
        assert torch.equal(alone[0].view(torch.int16), both[s].view(torch.int16)), f"{gn.id}: sample {s}"


# ------------------------------------------------------------------------------------------------------------------------------
# B. GroupNorm, producer statistics
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(s, k) for s in NC.ST_SHAPES for k in NC.KINDS[:4]], ids=lambda p: f"{p[0][0]}-{p[1]}")
def st(request, dev):
    """the input is produced as in test_groupnorm_with_producer_statistics: a K = 64 GEMM with ch_stats whose bias carries the offsets
    (sample 0's through `bias`, the other samples' difference to them through the per-sample `row_add`)"""
    from seva import ops
    (sid, hw, c1, c2), kind = request.param
    c = Case()
    c.id, c.kind, c.r, c.hw, c.c1, c.c2, c.C, c.n = f"{sid}-{kind}", kind, NC.rung_of(kind), hw, c1, c2, c1 + c2, NC.N
    off = NC.gn_offsets(kind, c.n, c.C, "producer").float()
    g = NC._gen("producer", sid, kind)

    def produce(ch, lo):
        a = torch.randn((c.n * hw, 64), generator=g).half().to(dev)
        w = (torch.randn((ch, 64), generator=g) / 8).half().to(dev)
        o = torch.full((c.n * hw, ch), NAN, device=dev)
        s = torch.full(ops.channel_stats_shape(c.n * hw, ch), NAN, device=dev)
        o_ch = off[:, lo:lo + ch]
        ops.gemm(a, w, bias=o_ch[0].contiguous().to(dev), row_add=(o_ch - o_ch[0]).contiguous().to(dev), rows_per_group=hw,
                 out_f32=o, ch_stats=s)
        return o.view(c.n, hw, ch), s

    c.x1, c.s1 = produce(c1, 0)
    c.x2, c.s2 = produce(c2, c1) if c2 else (None, None)
    torch.cuda.synchronize()
    c.x = torch.cat([c.x1.cpu(), c.x2.cpu()], -1) if c2 else c.x1.cpu()
    c.gamma, c.beta = NC.affine(c.C)
    c.gamma_d, c.beta_d = c.gamma.to(dev), c.beta.to(dev)
    c.ref = NC.gn_ref64(c.x, c.gamma, c.beta)
    _yardstick(c, NC.gn_torch32(c.x, c.gamma, c.beta))
    c.stats = torch.cat([c.s1.cpu(), c.s2.cpu()], 2) if c2 else c.s1.cpu()  # [n hw / 64][2][C]
    return c


def test_producer_statistics_are_fp32_block_sums(dev, st):
    """each block's sum and sum of squares against fp64 sums of the fp32 output: any fp32 summation order of 64 terms is within
    64 * 2^-24 of the sum of the terms' magnitudes (65 for the squares, which are rounded once more) -- relative to the sum itself
    where all terms share a sign, which is every block from r = 8 but for a rare channel whose offset came out small"""
    blk = st.x.double().view(st.n * st.hw // 64, 64, st.C)
    u = 2.0 ** -24
    d1 = (st.stats[:, 0].double() - blk.sum(1)).abs() / blk.abs().sum(1)
    d2 = (st.stats[:, 1].double() - (blk * blk).sum(1)).abs() / (blk * blk).sum(1)
    print(f"\n[producer statistics] {st.id}: block sums max error / sum|x| {float(d1.max()):.3e} (bound {64 * u:.3e}), "
          f"squares {float(d2.max()):.3e} (bound {65 * u:.3e})", flush=True)
    assert torch.isfinite(st.stats).all() and float(d1.max()) <= 64 * u and float(d2.max()) <= 65 * u


def _host_stats64(st):
    """mean, var [n, GROUPS] in fp64 from the fp32 block sums the producer wrote"""
    cpg = st.C // NC.GROUPS
    t = st.stats.double().view(st.n, st.hw // 64, 2, NC.GROUPS, cpg).sum((1, 4))  # [n][2][GROUPS]
    cnt = float(cpg * st.hw)
    mean = t[:, 0] / cnt
    return mean, (t[:, 1] / cnt - mean * mean).clamp_min(0.0)


def test_finalize_and_apply_given_the_statistics(dev, st):
    """gn_finalize_ch_kernel and the apply pass under ill-conditioning, independent of how good the statistics are"""
    got = _hi_lo(_run_gn(st, dev, split_out=True, stats=(st.s1, st.s2)), st.C)
    mean, var = _host_stats64(st)
    want = NC.gn_normalise64(st.x, mean, var, st.gamma, st.beta)
    err = NC.rel_l2(got, want)
    print(f"\n[producer statistics] {st.id} finalize + apply vs fp64 on the same block sums: e_torch {st.e_torch:.3e} e_fmt {st.e_fmt:.3e} "
          f"bound {st.bound:.3e} measured {err:.3e}", flush=True)
    assert torch.isfinite(got).all() and err < st.bound


def test_producer_statistics_end_to_end(dev, st):
    """against true fp64: the derived worst case of fp32 block sums (loose; catches a dropped block or a wrong count).  The f16
    readout's figures are printed, not asserted: they are the measured envelope of the producer path (norm section)"""
    got = _hi_lo(_run_gn(st, dev, split_out=True, stats=(st.s1, st.s2)), st.C)
    err, env = NC.rel_l2(got, st.ref), (1 + st.r ** 2) * 2.0 ** -18 + st.bound
    h = _run_gn(st, dev, silu=True, stats=(st.s1, st.s2)).cpu().double()
    ref = NC.silu_mod64(st.ref, True)
    e16, m16 = NC.rel_l2(h, ref), float((h - ref).abs().max() / ref.abs().max())
    print(f"\n[producer statistics] {st.id} end to end vs fp64: measured {err:.3e} (envelope {env:.3e}); f16 SiLU readout rel-L2 {e16:.3e} "
          f"max abs / max|ref| {m16:.3e}: {'meets' if e16 < 6e-4 and m16 < 2e-3 else 'EXCEEDS'} 6e-4 / 2e-3", flush=True)
    assert torch.isfinite(got).all() and err <= env
    # sample 1 alone, given its own blocks of the statistics, is bitwise sample 1 of the batch
    nb = st.hw // 64
    one = Case()
    one.__dict__.update(st.__dict__)
    one.n, one.x1, one.x2 = 1, st.x1[1:], st.x2[1:] if st.x2 is not None else None
    alone = _run_gn(one, dev, split_out=True, stats=(st.s1[nb:].contiguous(), st.s2[nb:].contiguous() if st.c2 else None))
    both = _run_gn(st, dev, split_out=True, stats=(st.s1, st.s2))
    assert torch.equal(alone[0].view(torch.int16), both[1].view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------------------
# C. LayerNorm
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(s, k) for s in NC.LN_SHAPES for k in NC.KINDS[:4]], ids=lambda p: f"{p[0][0]}-{p[1]}")
def ln(request, dev):
    (sid, rows, C), kind = request.param
    c = Case()
    c.id, c.rows, c.C = f"{sid}-{kind}", rows, C
    c.x = NC.ln_input(kind, rows, C)
    c.gamma, c.beta = NC.affine(C)
    c.ref = NC.ln_ref64(c.x, c.gamma, c.beta)
    _yardstick(c, NC.ln_torch32(c.x, c.gamma, c.beta))
    c.x_d, c.gamma_d, c.beta_d = c.x.to(dev), c.gamma.to(dev), c.beta.to(dev)
    return c


def test_layernorm_outputs(dev, ln):
    from seva import ops
    o32 = torch.full((ln.rows, ln.C), NAN, device=dev)
    osp = torch.full((ln.rows, 2 * ln.C), NAN, device=dev, dtype=F16)
    o16 = torch.full((ln.rows, ln.C), NAN, device=dev, dtype=F16)
    ops.layernorm(ln.x_d, ln.gamma_d, ln.beta_d, o32)
    ops.layernorm_split(ln.x_d, ln.gamma_d, ln.beta_d, osp)
    ops.layernorm(ln.x_d, ln.gamma_d, ln.beta_d, o16)
    torch.cuda.synchronize()
    e32, b32 = NC.rel_l2(o32.cpu(), ln.ref), NC.bound(ln.e_torch, 0.0)
    esp = NC.rel_l2(_hi_lo(osp, ln.C), ln.ref)
    h = o16.cpu().double()
    e16, m16 = NC.rel_l2(h, ln.ref), float((h - ln.ref).abs().max())
    print(f"\n[layernorm] {ln.id}: e_torch {ln.e_torch:.3e} e_fmt {ln.e_fmt:.3e}; fp32 measured {e32:.3e} (bound {b32:.3e}); "
          f"split measured {esp:.3e} (bound {ln.bound:.3e}); f16 rel-L2 {e16:.3e} (bound 6e-4) max abs {m16:.3e} (bound 4e-3)", flush=True)
    assert torch.isfinite(o32).all() and torch.isfinite(osp).all() and torch.isfinite(o16).all()
    assert e32 < b32
    assert esp < ln.bound
    assert e16 < 6e-4 and m16 < 4e-3
    assert torch.equal(osp[:, :ln.C], o16)  # the hi half is the plain f16 output


def test_ff_fused_layernorm_prologue_on_offset_rows(dev):
    """C = 320, M = 300 at r = 64: the fused feed-forward fed with LayerNorm's input against the same call fed with the separately
    normalised operand, under test_ff_fused_vs_two_kernels_and_fp32's tolerance for that pair"""
    from seva import ops
    from seva._engine import interleave_geglu
    M, C = 300, 320
    g = NC._gen("ff", M, C)
    w1 = (torch.randn(8 * C, C, generator=g) * C ** -0.5).half().to(dev)
    b1 = (0.3 * torch.randn(8 * C, generator=g)).to(dev)
    w2 = (torch.randn(C, 4 * C, generator=g) * (4 * C) ** -0.5).half().to(dev)
    b2 = (0.3 * torch.randn(C, generator=g)).to(dev)
    res = torch.randn(M, C, generator=g).to(dev)
    wi, bi = interleave_geglu(w1, b1)
    x = NC.ln_input("r64", M, C).to(dev)
    gm, bt = (t.to(dev) for t in NC.affine(C))
    a_ln = torch.empty((M, C), device=dev, dtype=F16)
    ops.layernorm(x, gm, bt, a_ln)
    want = torch.full((M, C), NAN, device=dev)
    ops.ff_fused(a_ln, wi, bi, w2, b2, residual=res, out_f32=want)
    got = torch.full((M, C), NAN, device=dev)
    ops.ff_fused(None, wi, bi, w2, b2, residual=res, out_f32=got, ln_x=x, ln_gamma=gm, ln_beta=bt)
    torch.cuda.synchronize()
    e_ln = NC.rel_l2(got, want)
    print(f"\n[ff_fused LayerNorm prologue] M = {M} C = {C} r = 64: vs the separately normalised operand {e_ln:.3e} (bound 2e-4)", flush=True)
    assert torch.isfinite(got).all() and e_ln < 2e-4
