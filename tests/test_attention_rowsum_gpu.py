"""attn16_kernel's softmax row sums come out of the matrix pipe (an A fragment of ones against the rounded P) and its rare "look at
the maximum" path is one wave-uniform branch per 64-key tile, decided per 16-row query block inside it.

Every case calls ops.attention with q_prescaled=True, the engine's call, and compares with an fp64 softmax on the f16 operands.
attn16_kernel<64> runs from lq >= ops.PV8_MIN_LQ (2048), attn16_kernel<64, true> + the combine from lk >= ops.ATTN_SPLIT_MIN_LK
(6144) with a workspace: the shapes are the smallest that reach each.  rel-L2 < 1e-3 is the project's bound for this kernel against
fp64 (tests/test_attn_norm_contract_gpu.py).

The constant-V bound 2^-10 is derived: numerator and denominator are fp32 sums of the same L <= 6177 non-negative terms, each within
L * 2^-24 = 3.7e-4 relative (worst case), so the quotient rounds to f16 within one f16 ulp at 1.0; a sum that missed a key block or
counted one twice is off by percent."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import rel_l2

F16, F64 = torch.float16, torch.float64
QK_C = 0.125 * 1.4426950408889634
KT = 64          # keys per tile
BOUND = 1e-3
STEP, JUMP = 48.0, 24.0   # the ramp of the rising / falling cases (log2 domain): per tile, and inside every odd tile


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from seva import _native
    _native.load()
    return torch.device("cuda:0")


def _run(q, k, v, split=False):
    """q: (B, lq, H * 64), k / v: (B, lk, H * 64), f16, q pre-scaled -> (B, lq, H * 64) f16"""
    from seva import ops
    B, lq, C = q.shape
    lk, H = k.shape[1], C // 64
    out = torch.full((B, lq, C), float("nan"), device=q.device, dtype=F16)
    ws = torch.empty(ops.attention_split_workspace_numel(B, H, lq), device=q.device) if split else None
    assert lq >= ops.PV8_MIN_LQ and (lk >= ops.ATTN_SPLIT_MIN_LK) == split, "the shape does not reach the kernel under test"
    ops.attention(q, k, v, out, nb0=B, nb1=1, heads=H, lq=lq, lk=lk, q_strides=(lq * C, 0, C), k_strides=(lk * C, 0, C),
                  o_strides=(lq * C, 0, C), q_prescaled=True, split_ws=ws)
    torch.cuda.synchronize()
    return out


def _scores64(q, k):
    B, lq, C = q.shape
    H = C // 64
    q4 = q.double().view(B, lq, H, 64).permute(0, 2, 1, 3)
    k4 = k.double().view(B, k.shape[1], H, 64).permute(0, 2, 1, 3)
    return q4 @ k4.transpose(-1, -2)  # (B, H, lq, lk), log2 domain


def _ref64(q, k, v):
    B, lq, C = q.shape
    H = C // 64
    s = _scores64(q, k)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    v4 = v.double().view(B, v.shape[1], H, 64).permute(0, 2, 1, 3)
    o = (p @ v4) / p.sum(-1, keepdim=True)
    return o.permute(0, 2, 1, 3).reshape(B, lq, C)


def _random(dev, B, H, lq, lk, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = (torch.randn(B, lq, H * 64, generator=g) * QK_C).to(dev, F16)
    k = torch.randn(B, lk, H * 64, generator=g).to(dev, F16)
    v = torch.randn(B, lk, H * 64, generator=g).to(dev, F16)
    return q, k, v


@pytest.mark.parametrize("what,B,H,lq,lk,split", [
    ("full_tiles", 1, 2, 2048, 2048, False),
    ("ragged", 1, 1, 2049, 2111, False),   # last workgroup: one live query row, three idle waves; last key tile: 63 keys, masked
    ("split", 1, 1, 6177, 6177, True),     # attn_write_partial16 + the combine
])
def test_random_against_fp64(dev, what, B, H, lq, lk, split):
    q, k, v = _random(dev, B, H, lq, lk, 11)
    out = _run(q, k, v, split)
    assert torch.isfinite(out).all()
    err = rel_l2(out, _ref64(q, k, v))
    print(f"{what}: rel-L2 {err:.3e}")
    assert err < BOUND, (what, err)


def _ramp_operands(dev, sign_rows=None):
    """lq = lk = 2048, one head.  Component 0 of every key is a ramp, +STEP per 64-key tile and +JUMP more on the last 16 keys of every odd
    tile; component 0 of a query is +1 (or sign_rows' -1): its score rises (falls) along the keys.  The other 63 components are small
    random numbers (|their part of the score| < 2)."""
    L = 2048
    g = torch.Generator(device="cpu").manual_seed(5)
    q = torch.randn(1, L, 64, generator=g) * QK_C
    k = torch.randn(1, L, 64, generator=g) * 0.25
    v = torch.randn(1, L, 64, generator=g)
    key = torch.arange(L)
    tile = key // KT
    ramp = STEP * tile + JUMP * ((tile % 2 == 1) & (key % KT >= 48))
    assert ramp.max() < 2048  # integers: exact in f16
    k[0, :, 0] = ramp
    q[0, :, 0] = 1.0 if sign_rows is None else sign_rows
    return q.to(dev, F16), k.to(dev, F16), v.to(dev, F16)


def _tile_maxima(s):
    return s.view(*s.shape[:-1], s.shape[-1] // KT, KT).amax(-1)


def test_rising_maximum(dev):
    """Every tile takes the rare path and P overflows f16 before the rescale (inf sums)."""
    q, k, v = _ramp_operands(dev)
    s = _scores64(q, k)
    tm = _tile_maxima(s)
    assert (tm[..., 1:] - tm[..., :-1]).min() > 16, "the case: every tile's maximum is more than 16 above the one before"
    st = s.view(1, 1, 2048, 2048 // KT, KT)
    assert ((st[..., 48:].amax(-1) - st[..., :48].amax(-1))[..., 1::2]).min() > 16, "the case: a rise of more than 16 inside odd tiles"
    out = _run(q, k, v)
    assert torch.isfinite(out).all()
    err = rel_l2(out, _ref64(q, k, v))
    print(f"rising: rel-L2 {err:.3e}")
    assert err < BOUND, err


def test_falling_maximum(dev):
    """The mirror: the same keys in reverse order, the rare path is never taken after tile 0."""
    q, k, v = _ramp_operands(dev)
    k, v = k.flip(1).contiguous(), v.flip(1).contiguous()
    tm = _tile_maxima(_scores64(q, k))
    assert (tm[..., 1:] - tm[..., :-1]).max() < -16
    out = _run(q, k, v)
    assert torch.isfinite(out).all()
    err = rel_l2(out, _ref64(q, k, v))
    print(f"falling: rel-L2 {err:.3e}")
    assert err < BOUND, err


def test_mixed_blocks(dev):
    """Of a wave's 64 queries only rows 16 .. 31 (one 16-row block) need a rescale on a tile: they see rising keys, the rest falling
    ones.  A merged branch that rescales or skips the wrong block fails here."""
    row = torch.arange(2048) % 64
    rising = (row >= 16) & (row < 32)
    sign = torch.where(rising, 1.0, -1.0)
    q, k, v = _ramp_operands(dev, sign)
    tm = _tile_maxima(_scores64(q, k))[0, 0]
    d = tm[:, 1:] - tm[:, :-1]
    assert d[rising.to(dev)].min() > 16 and d[~rising.to(dev)].max() < -16
    out = _run(q, k, v)
    assert torch.isfinite(out).all()
    ref = _ref64(q, k, v)
    for name, m in (("rising rows", rising), ("falling rows", ~rising)):
        err = rel_l2(out[0, m.to(dev)], ref[0, m.to(dev)])
        print(f"mixed, {name}: rel-L2 {err:.3e}")
        assert err < BOUND, (name, err)


@pytest.mark.parametrize("lq,lk,split", [(2049, 2111, False), (6177, 6177, True)])
def test_constant_v(dev, lq, lk, split):
    q, k, v = _random(dev, 1, 1, lq, lk, 3)
    v = torch.ones_like(v)
    out = _run(q, k, v, split)
    dev_max = float((out.float() - 1.0).abs().max())
    print(f"constant V, lk {lk}: max |out - 1| {dev_max:.3e}")
    assert dev_max <= 2.0 ** -10, dev_max


def test_nan_row(dev):
    """One query row of NaN: that output row is NaN, every other row of its wave is finite and inside the bound."""
    q, k, v = _random(dev, 1, 1, 2048, 2048, 7)
    r = 64 + 21  # wave 1 of the first workgroup, query block 1
    q[0, r] = float("nan")
    out = _run(q, k, v)
    assert torch.isnan(out[0, r]).all()
    keep = torch.ones(2048, dtype=torch.bool, device=dev)
    keep[r] = False
    assert torch.isfinite(out[0, keep]).all()
    qr = q.clone()
    qr[0, r] = 0
    ref = _ref64(qr, k, v)
    wave = torch.arange(64, 128, device=dev)
    wave = wave[wave != r]
    err_wave = rel_l2(out[0, wave], ref[0, wave])
    err_all = rel_l2(out[0, keep], ref[0, keep])
    print(f"NaN row: rel-L2 of its wave's other rows {err_wave:.3e}, of all finite rows {err_all:.3e}")
    assert err_wave < BOUND and err_all < BOUND, (err_wave, err_all)
