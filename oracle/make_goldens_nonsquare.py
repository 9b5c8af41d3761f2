"""Goldens at NON-SQUARE latents and at T=25 (dev container only; about ten minutes of CPU).

    PYTHONDONTWRITEBYTECODE=1 python oracle/make_goldens_nonsquare.py [--only g13_T8_72x96,...]

Sibling of `make_goldens_headline.py`: runs the REFERENCE (CPU fp32, imported read-only exactly as
`oracle/make_goldens.py` does) with the name-keyed synthetic 1.3B weights (seed 0) and the same
`[uncond; cond]` input recipe, generalised from one `HW` to `(h, w)`.  OUTPUTS only are stored -- every
input regenerates from `seva.synthetic` seeds (`nonsquare_inputs` below is mirrored in
tests/test_nonsquare_gpu.py):

  g13_T8_72x96_forward    one SGMWrapper call, T=8,  B=16, 768x576 px  (the Gradio guide's "basic" size)
  g13_T8_96x72_forward    same, portrait (576x768 px)
  g13_T8_72x128_forward   same, 16:9 (1024x576 px)
  g13_T25_72x72_forward   T=25, B=50 (the ViewCrafter evaluation recipe's frame count)

No committed file may exceed 1 MiB, so an output is stored in PARTS `<name>_forward_<k>.npz` of whole
latents, each with the row indices of its latents in the `[uncond; cond]` batch under `idx`.  The T = 8
outputs are stored whole (16 rows in 2 or 3 parts); of the T = 25 output the 25 conditional latents and the
unconditional latents 0, 12 and 24 (28 rows in 3 parts).

Reference call site: seva/model.py:176-234 (forward).
"""

from __future__ import annotations

import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as mg  # noqa: E402  (imports the reference + seva.synthetic)
from make_goldens_headline import full_net  # noqa: E402

rmodel, synth = mg.rmodel, mg.synth

# name -> (T, h, w, seed); x is drawn from seed + 1.  No collision with 400 / 500 / 600 / 701 / 702.
CASES = {
    "g13_T8_72x96": (8, 72, 96, 810),
    "g13_T8_96x72": (8, 96, 72, 820),
    "g13_T8_72x128": (8, 72, 128, 830),
    "g13_T25_72x72": (25, 72, 72, 840),
}
# rows of the [uncond; cond] batch that are stored (row T + i is conditional latent i)
STORED = {
    "g13_T8_72x96": list(range(16)),
    "g13_T8_96x72": list(range(16)),
    "g13_T8_72x128": list(range(16)),
    "g13_T25_72x72": [0, 12, 24] + list(range(25, 50)),
}
FILE_LIMIT = 1 << 20


def parts_of(rows, h, w):
    """`rows` cut into the fewest runs, of near-equal length, whose latents (4 x h x w fp32 each) fit one file"""
    per_file = (FILE_LIMIT - 8192) // (4 * h * w * 4)
    n = -(-len(rows) // per_file)
    q, r = divmod(len(rows), n)
    cuts = [0]
    for k in range(n):
        cuts.append(cuts[-1] + q + (k < r))
    return [rows[a:b] for a, b in zip(cuts, cuts[1:])]


def nonsquare_inputs(T, h, w, seed):
    """x (2T,4,h,w), t (2T,) int64, cond dict [uncond; cond] -- `make_goldens._wrapper_inputs` at (h, w)."""
    sc = synth.synth_scene(T, (h, w), (0,), seed=seed)
    x = mg.rnd(2 * T, 4, h, w, seed=seed + 1)
    c = {k: torch.cat((sc["uc"][k], sc["cond"][k]), 0) for k in ("crossattn", "concat", "dense_vector")}
    t = torch.full((2 * T,), 979, dtype=torch.int64)
    return x, t, c


@torch.no_grad()
def forward_golden(net, name):
    T, h, w, seed = CASES[name]
    x, t, c = nonsquare_inputs(T, h, w, seed)
    wrap = rmodel.SGMWrapper(net)
    t0 = time.time()
    y = wrap(x, t, c, num_frames=T)
    dt = time.time() - t0
    print(f"  reference 1.3B forward T={T}, {h}x{w}, B={2 * T}: {dt:.1f}s", flush=True)
    parts = parts_of(STORED[name], h, w)
    for k, rows in enumerate(parts):
        idx = torch.tensor(rows, dtype=torch.int64)
        mg.save(f"{name}_forward_{k}", y=y[idx], idx=idx, part=k, parts=len(parts), T=T, h=h, w=w, seed=seed, ref_seconds=dt,
                ref_threads=torch.get_num_threads())
        size = os.path.getsize(os.path.join(mg.GOLD, f"{name}_forward_{k}.npz"))
        assert size <= FILE_LIMIT, f"{name} part {k}: {size} bytes is over the limit for a committed file"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=",".join(CASES))
    args = ap.parse_args()
    want = set(args.only.split(","))
    t0 = time.time()
    net = full_net()
    print(f"  synth 1.3B weights loaded in {time.time() - t0:.1f}s", flush=True)
    for name in CASES:
        if name in want:
            forward_golden(net, name)


if __name__ == "__main__":
    main()
