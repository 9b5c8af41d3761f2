#!/usr/bin/env python3
"""Same-box, interleaved A/B of the long self-attention launches of one network call at T=21, 576x576: seva_attention_f16
(attn16_kernel) against the fp8 P.V path (seva_attn_quant_v_fp8 + seva_attention_pv8, each timed alone), on the packed [L, 3C]
q / k / v layout the engine hands them.  Prints microseconds per launch, best of the rounds."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "stable-virtual-camera_amd"))
import torch
from seva import ops

dev = torch.device("cuda:0")
QK_C = 0.125 * 1.4426950408889634
# (name, batch, heads, L, K/V split): per-frame 72x72 (42 frames), joint 36x36 and 18x18 (2 scenes x 21 frames)
SHAPES = [("frame 72x72", 42, 5, 5184, False), ("joint 36x36", 2, 10, 27216, True), ("joint 18x18", 2, 20, 6804, True)]
ROUNDS, REPS = int(os.environ.get("ROUNDS", "5")), int(os.environ.get("REPS", "5"))


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


for name, B, H, L, split in SHAPES:
    C = 64 * H
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B * L, 3 * C, generator=g)
    qkv[:, :C] *= QK_C
    qkv = qkv.half().to(dev)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    out = torch.empty(B * L, C, dtype=torch.float16, device=dev)
    ws = torch.empty(ops.v_fp8_workspace_numel(B, H, L), dtype=torch.uint8, device=dev)
    sws = torch.empty(ops.attention_split_workspace_numel(B, H, L), dtype=torch.float32, device=dev) if split else None
    kw = dict(nb0=B, nb1=1, heads=H, lq=L, lk=L, q_strides=(L * 3 * C, 0, 3 * C), k_strides=(L * 3 * C, 0, 3 * C),
              o_strides=(L * C, 0, C))
    f16 = lambda: ops.attention(q, k, v, out, q_prescaled=True, split_ws=sws, **kw)  # noqa: E731
    quant = lambda: ops.quantize_v_fp8(v, ws, nb0=B, nb1=1, heads=H, lk=L, k_strides=kw["k_strides"])  # noqa: E731
    pv8 = lambda: ops.attention_pv8(q, k, ws, out, split_ws=sws, **kw)  # noqa: E731
    quant()
    best = {"f16": 1e30, "quant": 1e30, "pv8": 1e30}
    for r in range(ROUNDS):  # interleaved: A, B, A, B, ...
        best["f16"] = min(best["f16"], timed(f16))
        best["quant"] = min(best["quant"], timed(quant))
        best["pv8"] = min(best["pv8"], timed(pv8))
    tot = best["quant"] + best["pv8"]
    print(f"{name:12s} B={B:2d} H={H:2d} L={L:5d} split={int(split)}: attn16 {best['f16']:8.1f} us | pv8 kernel {best['pv8']:8.1f} us "
          f"({100.0 * (best['pv8'] / best['f16'] - 1.0):+.1f} %) + V quantiser {best['quant']:6.1f} us = {tot:8.1f} us "
          f"({100.0 * (tot / best['f16'] - 1.0):+.1f} %)", flush=True)
