"""Whole-step hipGraph for `EulerEDMSampler.sampler_step` (north_star: "sampler loop captured in hipGraph").

One denoising step of either solver -- CFG input assembly, nearest-sigma lookup, the ~600 kernels of the CFG-batched
network call, denoiser combine, and then the solver's own part: noise perturbation, guidance and the Euler update
(reference seva/sampling.py:347-368 plus everything it calls), or guidance, the DPM-Solver++(2M) update and the new
history in one kernel -- is captured ONCE per trajectory into a hipGraph and replayed for the remaining steps.
Per-step values enter through static device buffers (sigma, next_sigma, x, and eps or the previous sigma), so the graph
is the step as a function, not a recording of one step's numbers.  The protocol -- eager warm-up, capture, fallback,
replay -- is `StepGraphCache.run`, the same for both solvers; they differ in the key, the closure and the fourth input.

PyTorch is used for what the task assigns to it -- device memory and streams: `torch.cuda.CUDAGraph` (= hipGraph on
ROCm) drives hipStreamBeginCapture / hipGraphInstantiate / hipGraphLaunch and gives the captured region a private
allocator pool, so the few host-sized torch ops inside the step (`torch.cat` of the cond dictionaries, the
argmin over the 1000-entry sigma table) keep stable addresses across replays.  All latent-sized math inside the
graph is libseva_hip.so kernels launched on the capturing stream.

What stays OUTSIDE the graph on purpose: the per-step Gaussian draw of the Euler step (`noise_fn`, default
`torch.randn_like`): the generator's Philox offset must advance per step exactly as in an eager run (and tests inject
recorded eps), so eps is drawn eagerly and copied into a static buffer -- graph and eager runs are bit-identical.  The
multistep solver's history buffer is not an input either: the captured kernel reads and writes it in place, by address.
"""

from __future__ import annotations

import os
import warnings

import torch

from . import _native


def enabled() -> bool:
    """SEVA_STEPGRAPH=0 disables whole-step capture (the network call alone is then replayed, SEVA_HIPGRAPH)."""
    return os.environ.get("SEVA_STEPGRAPH", "1") != "0" and os.environ.get("SEVA_HIPGRAPH", "1") != "0"


class StepGraph:
    """fn(*tensors) -> tensor, captured once; `inputs` are example tensors whose values are refreshed per replay."""

    def __init__(self, fn, inputs):
        dev = inputs[0].device
        # static buffers must be ordinary tensors even when the caller runs under torch.inference_mode()
        # (reference eval.py:1242): an inference tensor cannot be updated in place from outside that mode
        with torch.inference_mode(False):
            self.static_in = [torch.empty(t.shape, dtype=t.dtype, device=dev) for t in inputs]
        self._refresh(inputs)
        self.graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize(dev)
        # thread-local capture mode: HIP calls of OTHER threads (e.g. the RCCL watchdog of a multi-GPU job polling its events)
        # neither join nor invalidate this capture
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self.static_out = fn(*self.static_in)
        self.replays = 0

    def _refresh(self, inputs):
        for s, t in zip(self.static_in, inputs):
            s.copy_(t)

    def __call__(self, *inputs):
        self._refresh(inputs)
        self.graph.replay()
        self.replays += 1
        return self.static_out


class _Entry:
    """One key's place in the protocol: 0 = never seen, 1 = warmed; its graph once captured, and what that graph reads by address."""

    __slots__ = ("key", "state", "graph", "keep")

    def __init__(self):
        self.key, self.state, self.graph, self.keep = None, 0, None, None


class StepGraphCache:
    """One live graph per sampler and step kind: keyed by the identity of everything the captured step closes over.

    The key holds STRONG references (identity can then never be recycled by the allocator); a miss drops the old
    graph.  `state` per key: 0 = never seen -> run eagerly (warm-up: fills the engine arena, the guider's rule
    cache and every lazily packed weight; its result is the real step result), 1 = warmed -> capture + replay.

    The step kind (`run(..., kind=)`: 0 = a full step, L = a step whose network call is shallow at depth L, (0 or L, "unguided") =
    the same without guidance; any hashable value) is part of the key, and each kind has an entry of its own: a sampler that
    alternates full and shallow steps keeps both graphs alive, one that also leaves a guidance interval all four, at most four
    per window shape.  `key` / `state` / `graph` / `keep` name the full guided step's entry.
    """

    def __init__(self):
        self.entries: dict = {0: _Entry()}
        self.disabled = False
        self.captures = 0

    key = property(lambda self: self.entries[0].key)
    state = property(lambda self: self.entries[0].state)
    graph = property(lambda self: self.entries[0].graph)
    keep = property(lambda self: self.entries[0].keep)  # tensors of the warm-up step that the captured graph reads by address

    @staticmethod
    def flat_key(obj) -> tuple:
        """Flatten dict / tensor / scalar arguments into a tuple compared by identity (tensors, callables) or value."""
        if isinstance(obj, dict):
            out = []
            for k in sorted(obj):
                out.append(k)
                out.extend(StepGraphCache.flat_key(obj[k]))
            return tuple(out)
        if isinstance(obj, (list, tuple)):
            out = []
            for v in obj:
                out.extend(StepGraphCache.flat_key(v))
            return tuple(out)
        return (obj,)

    @staticmethod
    def _same(a, b) -> bool:
        if len(a) != len(b):
            return False
        for u, v in zip(a, b):
            if isinstance(u, (int, float, str, tuple, type(None))) or isinstance(v, (int, float, str, tuple, type(None))):
                if type(u) is not type(v) or u != v:
                    return False
            elif u is not v:
                return False
        return True

    def lookup(self, key, kind=0) -> _Entry:
        ent = self.entries.setdefault(kind, _Entry())
        if ent.key is None or not self._same(ent.key, key):
            ent.key, ent.state, ent.graph, ent.keep = key, 0, None, None
        return ent

    def reset(self):
        self.entries = {0: _Entry()}

    def run(self, key, fn, inputs, *, eligible, keep=None, kind=0):
        """One step `fn(*inputs)` under the protocol: eager while not `eligible`; else the first step of `key` eagerly, the
        second captured and replayed, every later one replayed.  `fn` is the sync-free step math, `inputs` the tensors whose
        values are refreshed per replay; `keep()`, read after a capture succeeded, is what the graph reads by address and the
        cache therefore holds for as long as the graph lives.  `kind`: the step kind, whose entry `key` is looked up in."""
        if not eligible:
            return fn(*inputs)
        ent = self.lookup(key, kind)
        if ent.state == 0:
            # warm-up = the real first step, launched eagerly (also without the network-only graph: it would be
            # captured for this one call only)
            with _native.eager_network():
                out = fn(*inputs)
            ent.state = 1
            return out
        if ent.graph is None:
            try:
                # capture records the step without running it: what `fn` updates in place is updated by the replays alone
                ent.graph = StepGraph(fn, inputs)
                self.captures += 1
                ent.keep = keep() if keep is not None else None
            except Exception as e:  # a step that cannot be captured (foreign denoiser with host syncs, ...) runs eagerly
                self.disabled = True
                self.reset()
                try:
                    torch.cuda.synchronize(inputs[0].device)
                except Exception:
                    pass
                warnings.warn(f"seva: whole-step hipGraph capture failed ({type(e).__name__}: {e}); "
                              "falling back to eager steps", RuntimeWarning)
                return fn(*inputs)
        # the graph's output buffer is overwritten by the next replay: hand the caller its own copy (435 KB)
        return ent.graph(*inputs).clone()
