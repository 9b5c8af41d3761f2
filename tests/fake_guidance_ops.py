"""TEST-ONLY torch emulation of `ops.cfg_rescale` (seva_cfg_rescale_f32, include/seva_hip.h), installed beside tests/fake_ops.py by
the CPU tests of the guidance controls.  Same contract as the kernel -- g as `fake_ops.cfg_combine` computes it, the four sums and
the multiplier in fp64, one rounding of m to fp32, one fp32 multiply -- but torch's summation order, not the kernel's tree: equal
to the kernel within the bounds of tests/test_guidance_gpu.py, not bit for bit.  Never imported by the product."""
import torch

import fake_ops


def rescale_multiplier(c, g, phi):
    """m[f] of the contract, fp64, from the cond half `c` and the guided latent `g` ((n, ...) fp32 tensors)."""
    n = c.shape[0]
    N = c[0].numel()
    cd, gd = c.reshape(n, -1).double(), g.reshape(n, -1).double()
    var_c = (cd * cd).sum(1) - cd.sum(1) ** 2 / N
    var_g = (gd * gd).sum(1) - gd.sum(1) ** 2 / N
    ok = (var_g > 0) & (var_c >= 0) if phi > 0 else torch.zeros(n, dtype=torch.bool)
    ratio = torch.where(ok, var_c / torch.where(ok, var_g, torch.ones_like(var_g)), torch.ones_like(var_g))
    return torch.where(ok, phi * torch.sqrt(ratio) + (1.0 - phi), torch.ones_like(var_g))


def cfg_rescale(den2, scale, phi, out, mult_out=None):
    if not 0.0 <= phi <= 1.0:
        raise ValueError(f"cfg_rescale: phi={phi} outside [0, 1]")
    assert den2.dtype == torch.float32 and out.dtype == torch.float32 and den2.shape[0] == 2 * out.shape[0]
    g = torch.empty_like(out)
    fake_ops.cfg_combine(den2, scale, g)
    phi = float(torch.tensor(phi, dtype=torch.float32))  # the ABI takes phi as a float
    m32 = rescale_multiplier(den2.chunk(2)[1], g, phi).float()
    out.copy_(m32.view(-1, *([1] * (g.ndim - 1))) * g)
    if mult_out is not None:
        mult_out.copy_(m32)
