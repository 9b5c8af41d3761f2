"""Shared by tests/test_norm_conditioning_cpu.py and tests/test_norm_conditioning_gpu.py: GroupNorm / LayerNorm inputs whose groups are
dominated by their offset (|mean| / std = r), the fp64 references and the yardstick every bound of the two files comes from.
Everything is seeded and built on the CPU, so both files see identical data.  Imports nothing of the product.

Why: var = E[x^2] - mean^2 summed in fp32 loses (1 + r^2) 2^-24 k of relative precision (k: a small factor of the summation order),
and the f16 output's own rounding floor (rel-L2 ~3e-4) hides that up to r ~ 64.  The ladder below walks r through 0, 8, 64, 512.

Yardstick: e_torch = rel-L2 of torch's fp32 CPU group_norm / layer_norm against fp64 on the case's own input, e_fmt = rel-L2 of
writing the fp64 reference in the output's format (an f16 [hi | lo] pair; 0 for fp32).  A near-fp32 readout must stay within
bound = 4 max(e_torch, e_fmt) + 1e-6: the factor 4 is what test_attn_norm_contract_gpu.py grants the fp32 LayerNorm, the floor is
16 fp32 roundings (16 * 2^-24) for the apply arithmetic and the hardware rsq / rcp where e_torch is one or two roundings itself."""
import zlib

import torch
import torch.nn.functional as F

GROUPS = 32
N = 2
RUNGS = (0, 8, 64, 512)
STRUCT_R = 64                    # the two extra structures sit on the r = 64 rung
KINDS = tuple(f"r{r}" for r in RUNGS) + ("spread", "const")
SPREAD_GROUP = 1                 # (a) group 1 of every sample: channels alternate +64 / -64 (well conditioned: real variance)
CONST_SAMPLE, CONST_GROUP, CONST_VALUE = 1, GROUPS - 1, 100.0   # (b) the last group of sample 1 is exactly 100.0
EPS = 1e-5
FLOOR = 16 * 2.0 ** -24          # 9.5e-7 < 1e-6

# id, hw, c1, c2: the smallest shapes that reach each path of csrc/norm.hip's statistics / apply passes
GN_SHAPES = (
    ("hw81_c64_16pixel_lanes_1slab", 81, 64, 0),
    ("hw324_c64", 324, 64, 0),
    ("hw1296_c320_quads_straddle_groups", 1296, 320, 0),
    ("hw324_c1280+640_512threads", 324, 1280, 640),
    ("hw81_c1280+1280_3zchunks", 81, 1280, 1280),
    ("hw37_c640+320_fewer_pixels_than_lanes", 37, 640, 320),
    ("hw20736_c128_vae_slab_cap", 20736, 128, 0),
)
# producer statistics (hw % 64 == 0)
ST_SHAPES = (
    ("hw64_c128_one_block", 64, 128, 0),
    ("hw1024_c320", 1024, 320, 0),
    ("hw256_c640+320", 256, 640, 320),
)
LN_SHAPES = (
    ("rows1000_c64", 1000, 64),
    ("rows1000_c320", 1000, 320),
    ("rows1000_c1280", 1000, 1280),
    ("rows65573_c320_four_rows_per_group", 65536 + 37, 320),
)


def rel_l2(a, b) -> float:
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def rung_of(kind: str) -> int:
    return int(kind[1:]) if kind[0] == "r" else STRUCT_R


def gn_offsets(kind: str, n: int, C: int, seed) -> torch.Tensor:
    """off[n, c] (fp64) = r s[n, g(c)] + randn, s = +-(1 + 0.25 randn): sign and size differ per group and per sample, the channels
    of a group differ by about one standard deviation of the pixel noise."""
    g = _gen("off", kind, n, C, seed)
    r = rung_of(kind)
    cpg = C // GROUPS
    sign = torch.randint(0, 2, (n, GROUPS), generator=g).double() * 2 - 1
    s = sign * (1 + 0.25 * torch.randn((n, GROUPS), generator=g, dtype=torch.float64))
    off = r * s.repeat_interleave(cpg, 1) + torch.randn((n, C), generator=g, dtype=torch.float64)
    if kind == "spread":
        c0 = SPREAD_GROUP * cpg
        alt = 64.0 * (1 - 2 * (torch.arange(cpg) % 2)).double()
        off[:, c0:c0 + cpg] = alt + torch.randn((n, cpg), generator=g, dtype=torch.float64)
    return off


def gn_input(kind: str, hw: int, C: int, n: int = N, seed=0):
    """-> (x [n, hw, C] fp32, off [n, C] fp64): x = fp32(off + randn)"""
    off = gn_offsets(kind, n, C, seed)
    x = (off[:, None, :] + torch.randn((n, hw, C), generator=_gen("x", kind, hw, C, n, seed), dtype=torch.float64)).float()
    if kind == "const":
        cpg = C // GROUPS
        x[CONST_SAMPLE, :, CONST_GROUP * cpg:(CONST_GROUP + 1) * cpg] = CONST_VALUE
    return x, off


def affine(C: int, seed=0):
    g = _gen("affine", C, seed)
    return 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


def modulation(n: int, hw: int, C: int, seed=0):
    """6-component modulation of test_groupnorm: (dense [n, hw, 6], dense_w [2C, 6], dense_b [2C])"""
    g = _gen("mod", n, hw, C, seed)
    return torch.randn((n, hw, 6), generator=g), 0.3 * torch.randn((2 * C, 6), generator=g), 0.1 * torch.randn(2 * C, generator=g)


def gn_normalise64(x, mean, var, gamma, beta, eps=EPS):
    """fp64 apply: x [n, hw, C], mean / var [n, GROUPS] (fp64)"""
    n, hw, C = x.shape
    xg = x.double().view(n, hw, GROUPS, C // GROUPS)
    y = (xg - mean[:, None, :, None]) / torch.sqrt(var[:, None, :, None] + eps)
    return y.view(n, hw, C) * gamma.double() + beta.double()


def gn_ref64(x, gamma, beta, eps=EPS):
    """fp64 GroupNorm(32) of x [n, hw, C] (channels last)"""
    n, hw, C = x.shape
    xg = x.double().view(n, hw, GROUPS, C // GROUPS)
    return gn_normalise64(x, xg.mean((1, 3)), xg.var((1, 3), unbiased=False), gamma, beta, eps)


def silu_mod64(y, silu: bool, mod=None):
    """SiLU and the modulation y (1 + scale) + shift on an fp64 GroupNorm result"""
    C = y.shape[-1]
    if silu:
        y = y * torch.sigmoid(y)
    if mod is not None:
        dmap, dw, db = mod
        d = dmap.double() @ dw.double().T + db.double()
        y = y * (1 + d[..., :C]) + d[..., C:]
    return y


def gn_torch32(x, gamma, beta, eps=EPS):
    """torch's own fp32 GroupNorm on the CPU (contiguous NCHW, its default kernel)"""
    y = F.group_norm(x.cpu().transpose(1, 2).contiguous(), GROUPS, gamma.cpu(), beta.cpu(), eps)
    return y.transpose(1, 2)


def ln_input(kind: str, rows: int, C: int, seed=0) -> torch.Tensor:
    """x[row, c] = fp32(r s[row] + randn), s = +-(1 + 0.25 randn): every row is offset-dominated by about r standard deviations"""
    g = _gen("ln", kind, rows, C, seed)
    sign = torch.randint(0, 2, (rows, 1), generator=g).double() * 2 - 1
    s = sign * (1 + 0.25 * torch.randn((rows, 1), generator=g, dtype=torch.float64))
    return (rung_of(kind) * s + torch.randn((rows, C), generator=g, dtype=torch.float64)).float()


def ln_ref64(x, gamma, beta, eps=EPS):
    return F.layer_norm(x.double(), (x.shape[-1],), gamma.double(), beta.double(), eps)


def ln_torch32(x, gamma, beta, eps=EPS):
    return F.layer_norm(x.cpu(), (x.shape[-1],), gamma.cpu(), beta.cpu(), eps)


def split_f16(ref64):
    """the fp64 reference written as an f16 [hi | lo] pair -> hi + lo in fp64"""
    hi = ref64.to(torch.float16)
    lo = (ref64 - hi.double()).to(torch.float16)
    return hi.double() + lo.double()


def e_fmt_split(ref64) -> float:
    return rel_l2(split_f16(ref64), ref64)


def bound(e_torch: float, e_fmt: float) -> float:
    return 4 * max(e_torch, e_fmt) + 1e-6


def const_group_tolerance(gamma, eps=EPS):
    """|y - beta| allowed in a group that is exactly CONST_VALUE: one fp32 ulp of the value (the rounding of the mean), amplified by
    eps^-1/2 |gamma|; per channel"""
    ulp = 2.0 ** (torch.tensor(CONST_VALUE).log2().floor().item() - 23)
    return ulp * eps ** -0.5 * gamma.double().abs()
