#!/usr/bin/env python3
"""Same-box, interleaved A/B of the ds1 feed-forward at the step's shape (C = 320, M = 217,728: T = 21, 72 x 72, both CFG halves):
ff_fused8_kernel<320> (seva_ff_fused_f16) against its e4m3 sibling (seva_ff_fused_fp8), both with the LayerNorm prologue and the
fp32 residual, as the engine launches them.  Prints microseconds per launch per round and the best of the rounds."""
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "stable-virtual-camera_amd"))
import torch  # noqa: E402

from seva import ops  # noqa: E402
from seva._engine import interleave_geglu  # noqa: E402

dev = torch.device("cuda:0")
C, M = 320, int(os.environ.get("M", "217728"))
ROUNDS, REPS = int(os.environ.get("ROUNDS", "5")), int(os.environ.get("REPS", "10"))


def timed(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / REPS


g = torch.Generator().manual_seed(0)
w1, b1 = interleave_geglu(torch.randn(8 * C, C, generator=g) / math.sqrt(C), torch.randn(8 * C, generator=g) * 0.1)
w2, b2 = torch.randn(C, 4 * C, generator=g) / math.sqrt(4 * C), torch.randn(C, generator=g) * 0.1
w1_8, w1_exp, w2_8, w2_exp = (t.to(dev) for t in ops.pack_ff_fp8(w1.float(), w2))
w1h, w2h = w1.half().to(dev).contiguous(), w2.half().to(dev).contiguous()
b1, b2 = b1.float().to(dev), b2.to(dev)
x = torch.randn(M, C, device=dev)
res = torch.randn(M, C, device=dev)
gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
out = torch.empty(M, C, device=dev)
ln = dict(ln_x=x, ln_gamma=gamma, ln_beta=beta, ln_eps=1e-5)
f16 = lambda: ops.ff_fused(None, w1h, b1, w2h, b2, residual=res, out_f32=out, **ln)  # noqa: E731
fp8 = lambda: ops.ff_fused_fp8(None, w1_8, w1_exp, b1, w2_8, w2_exp, b2, residual=res, out_f32=out, **ln)  # noqa: E731
flop = 2.0 * M * C * 8 * C + 2.0 * M * 4 * C * C
best = {"f16": 1e30, "fp8": 1e30}
for r in range(ROUNDS):  # interleaved: A, B, A, B, ...
    t16, t8 = timed(f16), timed(fp8)
    best["f16"], best["fp8"] = min(best["f16"], t16), min(best["fp8"], t8)
    print(f"round {r}: ff_fused8_kernel<320> {t16:8.1f} us | ff_fused8_fp8_kernel<320> {t8:8.1f} us ({t16 / t8:.3f}x)", flush=True)
print(f"best of {ROUNDS}: f16 {best['f16']:.1f} us ({flop / best['f16'] * 1e-6:.0f} TFLOP/s) | fp8 {best['fp8']:.1f} us "
      f"({flop / best['fp8'] * 1e-6:.0f} TFLOP/s): {best['f16'] / best['fp8']:.3f}x; x15 per step: "
      f"{15 * (best['f16'] - best['fp8']) / 1000.0:+.2f} ms saved", flush=True)
