"""Device time of the dynamic-range audit (profiles/range_audit.log; DESIGN.md quotes it).

  1. seva_tensor_range beside torch's own one-pass reduction `x.abs().max()` on the same tensor (an independent streaming read,
     not the code under test), at the largest tensors an audited T = 21, 576 x 576 step sees: [217728, 2560] f16 (the unfused GEGLU
     hidden, 1.11 GB), [217728, 320] f32, and the e4m3 tensor of the first size.  The two candidates alternate in one process,
     REPS times each after a warm-up, timed with device events; median, min and max are printed.  Target: no slower than the
     reduction plus the spread the reduction itself shows.
  2. One eager T = 21, 576 x 576 call of the 1.3 B network under `audit.record()` over the same eager call without it, and the
     number of records (no threshold).  --no-network skips it.

Run from the repository root on an MI355X:  python tools/krange_time.py"""
import argparse
import statistics
import sys

import torch

sys.path[:0] = ["stable-virtual-camera_amd", "tests", "."]
from seva import audit, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--rows", type=int, default=217728)
ap.add_argument("--no-network", action="store_true")
args = ap.parse_args()
REPS = max(5, args.reps)
HBM_PEAK = 8.0e12  # bytes / s, HBM3E peak of the MI355X
dev = torch.device("cuda:0")
F16, F32, U8 = torch.float16, torch.float32, torch.uint8


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(a, b):
    for _ in range(2):  # warm-up: code objects, allocator, algorithm choice
        a()
        b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(REPS):
        ta.append(timed(a))
        tb.append(timed(b))
    return ta, tb


def fmt(ts):
    return f"median {statistics.median(ts):.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})"


def make(rows, cols, dtype):
    g = torch.Generator(device=dev).manual_seed(rows + cols)
    x = torch.empty((rows, cols), dtype=dtype, device=dev)
    step = 16384
    for r in range(0, rows, step):  # activations: a few binades around 1, some exact zeros
        v = torch.randn((min(step, rows - r), cols), generator=g, device=dev) * 4.0
        v[:, ::17] = 0.0
        x[r:r + step] = ops.to_fp8(v) if dtype == U8 else v.to(dtype)
    return x


print(f"seva_tensor_range vs torch x.abs().max(), {REPS} alternating repeats each, device events", flush=True)
for cols, dtype, name in ((2560, F16, "f16"), (320, F32, "f32"), (2560, U8, "e4m3")):
    x = make(args.rows, cols, dtype)
    nbytes = x.numel() * x.element_size()
    out = torch.empty(ops.RANGE_WORDS, dtype=torch.int64, device=dev)
    ws = torch.empty(ops.tensor_range_workspace_numel(*x.shape), dtype=U8, device=dev)
    yard, what = (lambda: x.abs().max()), "x.abs().max()"
    if dtype == U8:
        x8 = x.view(torch.float8_e4m3fn)
        try:
            x8.abs().max()
            yard, what = (lambda: x8.abs().max()), "x.view(float8_e4m3fn).abs().max()"
        except Exception as e:  # torch without the float8 reduction: the same bytes through the integer maximum
            yard, what = (lambda: x.max()), f"x.max() on the bytes (float8 abs().max() unavailable: {type(e).__name__})"
    t_k, t_y = alternate(lambda: ops.tensor_range(x, out, workspace=ws), yard)
    mk, my = statistics.median(t_k), statistics.median(t_y)
    spread = max(t_y) - min(t_y)
    w = out.tolist()
    print(f"[{args.rows}, {cols}] {name} ({nbytes / 1e9:.3f} GB): tensor_range {fmt(t_k)} = {nbytes / mk / 1e6:.0f} GB/s, "
          f"{100 * nbytes / (mk * 1e-3) / HBM_PEAK:.1f} % of the 8 TB/s HBM peak | {what} {fmt(t_y)} = {nbytes / my / 1e6:.0f} GB/s | "
          f"ratio {mk / my:.2f}, target (reduction + its spread {spread:.3f} ms) {'met' if mk <= my + spread else 'MISSED'}; "
          f"words: zeros {w[0]}, inf {w[65]}, nan {w[66]}, at_max {w[67]}, sum identity {w[0] + sum(w[1:65]) + w[65] + w[66] == w[70]}",
          flush=True)
    del x, out, ws

if not args.no_network:
    from test_model_gpu import _build  # the synthetic 1.3 B network of the GPU tests

    net, _ = _build("full", dev)
    eng = net.engine()
    eng.use_graph = False
    T, hw = 21, 72
    n = 2 * T
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(n, 4, hw, hw, generator=g) * 10).to(dev)
    concat = torch.randn(n, 7, hw, hw, generator=g).to(dev)
    t = torch.full((n,), 700, dtype=torch.int64, device=dev)
    y = torch.randn(n, 1, 1024, generator=g).to(dev)
    dense = torch.randn(n, 6, hw * 8, hw * 8, generator=g).to(dev)

    def plain():
        return eng.forward(x, concat, t, y, dense, T)

    recs = []

    def audited():
        with audit.record() as rec:
            o = eng.forward(x, concat, t, y, dense, T)
        recs.append(rec)
        return o

    ref = plain().clone()
    t_a, t_p = alternate(audited, plain)
    same = torch.equal(audited(), ref)
    rep = recs[-1].report()
    print(f"eager T = 21, 576 x 576 network call: plain {fmt(t_p)}, under audit.record() {fmt(t_a)}, ratio "
          f"{statistics.median(t_a) / statistics.median(t_p):.2f}; {len(rep.rows)} records, "
          f"{sum(r.count * {'f32': 4, 'f16': 2, 'e4m3': 1}[r.dtype] for r in rep.rows) / 1e9:.2f} GB audited; output bit-equal {same}; "
          f"first non-finite: {rep.first_nonfinite()}", flush=True)
    print("least headroom:\n" + rep.table(rep.worst(5)), flush=True)
