"""Torch emulation of the three LPIPS operators (`ops.lpips_prepare`, `ops.lpips_relu_pool`, `ops.lpips_layer`) for the CPU tests:
the arithmetic contract of include/seva_hip.h restated operation by operation in fp32 torch -- separate multiplies, adds and
divisions in the stated order, the xor-butterflies over a pixel's lanes, the fp64 trees over a chunk's threads and a pair's chunks
-- so that `seva._lpips_engine` runs without a GPU (`OPS`: these beside tests/fake_ops.py's convolution) and the contract itself
can be held against fp64.  Divisors are full tensors, never Python scalars: a true fp32 division per element.  The square root
is taken in fp64 and rounded once to fp32, which is the correctly rounded fp32 root (53 >= 2 * 24 + 2 bits): torch's own fp32
`sqrt` on the CPU is not correctly rounded in every build (a vector-library routine: 0.6 % of the values differ by an ulp)."""
import types

import torch

import fake_frame_ops
import fake_ops

F16, F32, F64 = torch.float16, torch.float32, torch.float64
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
THREADS = PIXELS = 256
LPIPS_CPAD = 64


def prepared(u8: torch.Tensor) -> torch.Tensor:
    """uint8 (n,H,W,3) -> f16 (n,H,W,3): x = float(u) / 127.5f; x - 1.0f; x - shift[c]; x / scale[c]; one RNE to f16."""
    x = u8.to(F32)
    x = x / torch.full_like(x, 127.5)
    x = x - torch.ones_like(x)
    x = x - torch.tensor(SHIFT, dtype=F32).expand_as(x)
    x = x / torch.tensor(SCALE, dtype=F32).expand_as(x).contiguous()
    return x.to(F16)


def lpips_prepare(x, out_f16):
    out_f16.zero_()
    out_f16[..., :3] = prepared(fake_frame_ops.as_u8(x))


def lpips_relu_pool(x, relu_out, pool_out=None):
    n, h, w, c = x.shape
    assert c % 64 == 0
    zero = torch.zeros((), dtype=F16)
    r = torch.where(x <= zero, zero, x)  # NaN <= 0 is false: a NaN stays
    relu_out.copy_(r)
    if pool_out is not None:
        m = None
        for dy in range(2):
            for dx in range(2):
                v = r[:, dy:2 * (h // 2):2, dx:2 * (w // 2):2]
                m = v if m is None else torch.where((v > m) | torch.isnan(v), v, m)
        pool_out.copy_(m)


def lpips_layer_workspace_numel(n, hw):
    return n * ((hw + PIXELS - 1) // PIXELS) * 8


def _tree(v):
    """v[..., t] += v[..., t + s] for s = 128 .. 1 over 256 fp64 values -> v[..., 0]"""
    v = v.clone()
    s = THREADS // 2
    while s:
        v[..., :s] = v[..., :s] + v[..., s:2 * s]
        s //= 2
    return v[..., 0]


def _sqrt_rn(x):
    return torch.sqrt(x.to(F64)).to(F32)


def pixel_distance_f32(fa, fb, w):
    """f16 (n,hw,C) x 2, fp32 (C) -> fp32 (n,hw): the per-pixel d of the contract."""
    n, hw, C = fa.shape
    L = C // 8
    a, b, wv = fa.to(F32).view(n, hw, L, 8), fb.to(F32).view(n, hw, L, 8), w.view(L, 8)
    lane = torch.arange(L)

    def butterfly(s):
        o = L // 2
        while o:
            s = s + s[..., lane ^ o]
            o //= 2
        return s

    def recip_norm(v):
        s = torch.zeros((n, hw, L), dtype=F32)
        for i in range(8):
            s = s + v[..., i] * v[..., i]
        nrm = _sqrt_rn(butterfly(s)) + torch.full((n, hw, L), 1e-10, dtype=F32)
        return torch.ones_like(nrm) / nrm

    ra, rb = recip_norm(a), recip_norm(b)
    d = torch.zeros((n, hw, L), dtype=F32)
    for i in range(8):
        df = a[..., i] * ra - b[..., i] * rb
        d = d + wv[:, i] * (df * df)
    return butterfly(d)[..., 0]


def lpips_layer(fa, fb, w, out, workspace=None):
    n, hw, C = fa.shape
    assert C in (64, 128, 256, 512) and fa.dtype == fb.dtype == F16 and w.dtype == F32 and out.dtype == F64
    L = C // 8
    G = THREADS // L
    chunks = (hw + PIXELS - 1) // PIXELS
    d = torch.zeros((n, chunks * PIXELS), dtype=F64)  # (a pixel beyond the frame adds nothing: + 0.0 is exact)
    d[:, :hw] = pixel_distance_f32(fa, fb, w).to(F64)
    d = d.view(n, chunks, PIXELS // G, G)
    acc = torch.zeros((n, chunks, G), dtype=F64)
    for k in range(PIXELS // G):  # thread g * L: pixels g, g + G, ... of the chunk, in order
        acc = acc + d[:, :, k]
    v = torch.zeros((n, chunks, THREADS), dtype=F64)
    v[..., ::L] = acc
    part = _tree(v)  # (n, chunks)
    rounds = (chunks + THREADS - 1) // THREADS
    p = torch.zeros((n, rounds * THREADS), dtype=F64)
    p[:, :chunks] = part
    p = p.view(n, rounds, THREADS)
    s = torch.zeros((n, THREADS), dtype=F64)
    for r in range(rounds):  # thread t: chunks t, t + 256, ...
        s = s + p[:, r]
    out.copy_(_tree(s))


# the operator namespace of `seva._lpips_engine` on the CPU
OPS = types.SimpleNamespace(conv3x3=fake_ops.conv3x3, lpips_prepare=lpips_prepare, lpips_relu_pool=lpips_relu_pool,
                            lpips_layer=lpips_layer, lpips_layer_workspace_numel=lpips_layer_workspace_numel)
