"""TEST-ONLY torch restatement of seva_tensor_range (include/seva_hip.h): the 72-word contract computed from the elements' bit
patterns with integer tensor operations only (no floating-point instruction sees a value, as in the kernel).  Runs on whatever
device the tensor is on.  tests/test_range_cpu.py holds it against an independent derivation (torch.frexp on fp64); the GPU
tests compare the kernel with it word for word.  Never imported by the product."""
import torch

from seva.ops import RANGE_MAX_WGS as MAX_WGS, RANGE_WG_ELEMS as WG_ELEMS, RANGE_WORDS as WORDS

INF32 = 0x7F800000
FMT_MAX_BITS = {torch.float32: 0x7F7FFFFF, torch.float16: 0x7BFF, torch.uint8: 0x7E}


def workgroups(total: int) -> tuple[int, int]:
    """(elements per workgroup, workgroups) of the counting kernel for `total` elements."""
    share = WG_ELEMS
    if total > WG_ELEMS * MAX_WGS:
        share = -(-(-(-total // MAX_WGS)) // WG_ELEMS) * WG_ELEMS
    return share, -(-total // share)


def tensor_range_workspace_numel(rows: int, cols: int) -> int:
    return workgroups(rows * cols)[1] * WORDS * 8


def _msb(m: torch.Tensor, bits: int) -> torch.Tensor:
    """floor(log2 m) of positive integers below 2^bits."""
    r = torch.zeros_like(m)
    for j in range(1, bits):
        r += (m >= (1 << j)).to(m.dtype)
    return r


def magnitude_bits(x: torch.Tensor) -> torch.Tensor:
    if x.dtype == torch.float32:
        return x.contiguous().view(torch.int32).to(torch.int64) & 0x7FFFFFFF
    if x.dtype == torch.float16:
        return x.contiguous().view(torch.int16).to(torch.int64) & 0x7FFF
    assert x.dtype == torch.uint8
    return x.to(torch.int64) & 0x7F


def classify(m: torch.Tensor, dtype):
    """(zero, inf, nan masks; bin k of the finite non-zero elements; f32 bit pattern of every finite |x|), all from m."""
    if dtype == torch.float32:
        zero, inf, nan = m == 0, m == INF32, m > INF32
        k = ((m >> 23) - 95).clamp(0, 63)
        f32 = m
    else:
        mb, eb, bias = (10, 5, 15) if dtype == torch.float16 else (3, 4, 7)
        top = (1 << eb) - 1
        E, frac = m >> mb, m & ((1 << mb) - 1)
        zero = m == 0
        if dtype == torch.float16:
            inf, nan = (E == top) & (frac == 0), (E == top) & (frac != 0)
        else:  # e4m3 "fn": no infinity, the all-ones pattern is the NaN
            inf, nan = torch.zeros_like(zero), m == 0x7F
        msb = _msb(m.clamp_min(1), mb)
        sub = E == 0
        e = torch.where(sub, msb - (bias - 1) - mb, E - bias)  # subnormal: m * 2^(1 - bias - mb)
        k = (e + 32).clamp(0, 63)
        # f32 bits: exponent e + 127, the mb (normal) or msb (subnormal) fraction bits moved to the top of the 23
        f_norm = ((E - bias + 127) << 23) | (frac << (23 - mb))
        f_sub = ((e + 127) << 23) | ((m ^ (1 << msb)) << (23 - msb))
        f32 = torch.where(sub, f_sub, f_norm)
    return zero, inf, nan, k, f32


def tensor_range(x, out=None, *, rows=None, cols=None, workspace=None):
    if x.dim() == 1:
        x = x.unsqueeze(0)
    assert x.dim() == 2
    rows = x.shape[0] if rows is None else rows
    cols = x.shape[1] if cols is None else cols
    m = magnitude_bits(x[:rows, :cols]).reshape(-1)
    zero, inf, nan, k, f32 = classify(m, x.dtype)
    fin = ~(zero | inf | nan)
    w = torch.zeros(WORDS, dtype=torch.int64, device=x.device)
    w[0] = zero.sum()
    w[1:65] = torch.bincount(k[fin], minlength=64)
    w[65], w[66] = inf.sum(), nan.sum()
    w[67] = (m == FMT_MAX_BITS[x.dtype]).sum()
    w[68] = f32[fin].max() if bool(fin.any()) else 0
    w[69] = f32[fin].min() if bool(fin.any()) else INF32
    w[70] = rows * cols
    if out is None:
        return w
    out.copy_(w)
    return out
