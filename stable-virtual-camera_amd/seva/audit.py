"""Dynamic-range audit: which launch overflowed, and how much headroom the others have.

The hot path carries activations as f16 (and, in the fp8 modes, as e4m3); f16 producers write inf above 65504 and e4m3
producers saturate at +-448.  With a real checkpoint one activation outside the range is enough for NaN
latents and black frames.  This module runs `ops.tensor_range` (one pass: exact exponent histogram, zero / inf / NaN / at-max
counts, finite extrema) over every floating-point output that `seva.ops` writes while a recorder is active:

    from seva import audit
    with audit.record() as rec:          # eager launches; raises inside a stream capture; no nesting
        out = model(x, t, c)             # or ae.decode(z), conditioner(img), a whole sampler call, pipeline.run_window(...)
    rep = rec.report()                   # the one host sync
    print(rep.first_nonfinite())         # the launch that produced the first inf / NaN
    print(rep.table(rep.worst(10)))      # the launches closest to the f16 / e4m3 limit

Under a recorder everything launches eagerly: the engines skip their network graphs and the sampler neither captures nor replays its
whole-step graph, so every step of a sampler call is recorded; graphs captured earlier are replayed again afterwards.

Off by default: without a recorder (and without SEVA_AUDIT / SEVA_CHECK_FINITE) the library makes exactly the calls it made
before.  What the audit cannot see: tensors that never reach HBM (the GEGLU hidden inside the fused feed-forward, attention
scores); an overflow there shows as the first non-finite OUTPUT, and the report names that launch.
"""

from __future__ import annotations

import functools
import json
import math
import os
import weakref

import torch

from . import _native, ops

WORDS = ops.RANGE_WORDS
CHUNK = 1024  # records per device table; the recorder grows by whole tables (no copy, no sync)
DTYPE_NAMES = {torch.float32: "f32", torch.float16: "f16", torch.uint8: "e4m3"}
# format -> (largest finite value, exponent of the smallest normal, exponent of the largest finite value)
FORMATS = {"f32": (3.4028234663852886e38, -126, 127), "f16": (65504.0, -14, 15), "e4m3": (448.0, -6, 8)}

_ARENAS: "weakref.WeakSet" = weakref.WeakSet()  # every engine arena alive (`_Arena` registers itself)


def register_arena(arena) -> None:
    _ARENAS.add(arena)


def _bits_to_float(bits: int) -> float:
    return float(torch.tensor([bits], dtype=torch.int64).to(torch.int32).view(torch.float32)[0])


class Row:
    """One audited output of one launch."""

    FIELDS = ("seq", "scope", "op", "output", "buffer", "dtype", "rows", "cols", "zeros", "inf", "nan", "at_max", "max_abs",
              "min_abs", "hist")

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, kw[f])

    @classmethod
    def from_words(cls, words, **meta) -> "Row":
        w = [int(v) & 0xFFFFFFFFFFFFFFFF for v in words]
        return cls(zeros=w[0], hist=w[1:65], inf=w[65], nan=w[66], at_max=w[67], max_abs=_bits_to_float(w[68]),
                   min_abs=_bits_to_float(w[69]), **meta)

    @property
    def count(self) -> int:
        return self.rows * self.cols

    @property
    def finite_nonzero(self) -> int:
        return sum(self.hist)

    def consistent(self) -> bool:
        """The sum identity of word [70]."""
        return self.zeros + sum(self.hist) + self.inf + self.nan == self.count

    def _fmt(self, fmt):
        fmt = fmt or ("f16" if self.dtype == "f32" else self.dtype)
        if fmt not in FORMATS:
            raise ValueError(f"unknown format {fmt!r} (one of {sorted(FORMATS)})")
        return fmt

    def headroom_bits(self, fmt: str | None = None) -> float:
        """log2(largest finite value of `fmt` / max_abs); fmt defaults to the row's dtype, for f32 rows to "f16" ("if this were
        cast to f16").  inf for a tensor without a finite non-zero element."""
        fmax = FORMATS[self._fmt(fmt)][0]
        return math.inf if self.max_abs == 0.0 else math.log2(fmax / self.max_abs)

    def subnormal_share(self, fmt: str | None = None) -> float:
        """Share of the finite non-zero elements below the smallest normal of `fmt` (f16: e < -14, e4m3: e < -6)."""
        emin = FORMATS[self._fmt(fmt)][1]
        if emin < -32:
            raise ValueError("the table ends at 2^-32: subnormal_share is defined for f16 and e4m3")
        n = self.finite_nonzero
        return sum(self.hist[: emin + 32]) / n if n else 0.0

    def above_share(self, fmt: str | None = None) -> float:
        """Share of the finite non-zero elements in bins above the top exponent of `fmt` (f16: e > 15, e4m3: e > 8)."""
        emax = FORMATS[self._fmt(fmt)][2]
        if emax > 31:
            raise ValueError("the table ends at 2^31: above_share is defined for f16 and e4m3")
        n = self.finite_nonzero
        return sum(self.hist[emax + 33:]) / n if n else 0.0

    def to_dict(self) -> dict:
        d = {f: getattr(self, f) for f in self.FIELDS}
        d["max_abs"], d["min_abs"] = float(self.max_abs).hex(), float(self.min_abs).hex()  # exact through JSON
        return d

    @classmethod
    def from_dict(cls, d: dict) -> "Row":
        d = dict(d)
        d["max_abs"], d["min_abs"] = float.fromhex(d["max_abs"]), float.fromhex(d["min_abs"])
        return cls(**d)

    def __eq__(self, other):
        return isinstance(other, Row) and self.to_dict() == other.to_dict()

    def __repr__(self):
        return (f"Row(seq={self.seq}, scope={self.scope!r}, op={self.op!r}, output={self.output!r}, buffer={self.buffer!r}, "
                f"dtype={self.dtype}, {self.rows}x{self.cols}, max_abs={self.max_abs:.6g}, inf={self.inf}, nan={self.nan}, "
                f"at_max={self.at_max})")


class Report:
    def __init__(self, rows):
        self.rows = list(rows)

    def first_nonfinite(self) -> Row | None:
        """The lowest-seq row with an inf or a NaN: the launch to look at."""
        bad = [r for r in self.rows if r.inf + r.nan > 0]
        return min(bad, key=lambda r: r.seq) if bad else None

    def worst(self, k: int = 10, fmt: str | None = None) -> list:
        """The k rows with the least headroom in `fmt` (each row's own format by default), non-finite rows first."""
        return sorted(self.rows, key=lambda r: (r.inf + r.nan == 0, r.headroom_bits(fmt), r.seq))[:k]

    def table(self, rows=None, fmt: str | None = None) -> str:
        rows = self.rows if rows is None else rows
        head = f"{'seq':>5} {'scope':<44} {'op':<22} {'output':<12} {'buffer':<16} {'dtype':<5} {'elements':>11} " \
               f"{'max_abs':>11} {'headroom':>8} {'sub%':>6} {'inf':>8} {'nan':>8} {'at_max':>8}"
        lines = [head]
        for r in rows:
            f = r._fmt(fmt)
            sub = 100.0 * r.subnormal_share(f) if FORMATS[f][1] >= -32 else float("nan")
            lines.append(f"{r.seq:>5} {r.scope:<44} {r.op:<22} {r.output:<12} {r.buffer:<16} {r.dtype:<5} {r.count:>11} "
                         f"{r.max_abs:>11.4g} {r.headroom_bits(fmt):>8.2f} {sub:>6.2f} {r.inf:>8} {r.nan:>8} {r.at_max:>8}")
        return "\n".join(lines)

    def to_dict(self) -> dict:
        return {"rows": [r.to_dict() for r in self.rows]}

    def to_json(self, path: str) -> None:
        with open(path, "w") as f:
            json.dump(self.to_dict(), f)

    @classmethod
    def from_dict(cls, d: dict) -> "Report":
        return cls(Row.from_dict(r) for r in d["rows"])

    @classmethod
    def from_json(cls, path: str) -> "Report":
        with open(path) as f:
            return cls.from_dict(json.load(f))


def _capturing() -> bool:
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class Recorder:
    """Collects one 72-word table per audited output on the device; `report()` is the only host sync."""

    def __init__(self):
        self.scope = ""
        self._meta: list = []    # (scope, op, output, arena key, dtype name, rows, cols)
        self._tables: list = []  # [CHUNK][72] int64, device memory
        self._ws = None
        self._eager = _native.eager_network()
        self._open = False

    def __enter__(self) -> "Recorder":
        if ops._AUDIT is not None:
            raise _native.SevaNativeError("audit.record(): a recorder is already active (recorders do not nest)")
        if _capturing():
            raise _native.SevaNativeError("audit.record(): the current stream is capturing a graph; the audit needs eager launches")
        self._eager.__enter__()  # the engines launch eagerly instead of replaying their graphs
        ops._AUDIT = self
        self._open = True
        return self

    def __exit__(self, *exc):
        ops._AUDIT = None
        self._open = False
        self._eager.__exit__(*exc)
        return False

    def output(self, op: str, label: str, t: torch.Tensor, off: int, rows: int, cols: int, pitch: int) -> None:
        """One written area of one launch: rows x cols elements at element offset `off` of t, rows `pitch` apart."""
        if t.dtype not in DTYPE_NAMES or rows <= 0 or cols <= 0:
            return
        if _capturing():
            raise _native.SevaNativeError("audit: a graph capture began while a recorder is active")
        i = len(self._meta)
        if i % CHUNK == 0:
            self._tables.append(torch.zeros((CHUNK, WORDS), dtype=torch.int64, device=t.device))
        view = t.as_strided((rows, cols), (pitch if rows > 1 else cols, 1), t.storage_offset() + off)
        need = ops.tensor_range_workspace_numel(rows, cols)
        if self._ws is None or self._ws.numel() < need or self._ws.device != t.device:
            self._ws = torch.empty(max(need, 1 << 20), dtype=torch.uint8, device=t.device)  # (launches of one stream: reuse is ordered)
        ops.tensor_range(view, self._tables[-1][i % CHUNK], workspace=self._ws)
        first = view.data_ptr()
        self._meta.append((self.scope, op, label, _arena_key(first, first + ((rows - 1) * pitch + cols) * t.element_size()),
                           DTYPE_NAMES[t.dtype], rows, cols))

    def __len__(self):
        return len(self._meta)

    def report(self) -> Report:
        """Copies the device tables: the one host sync.  (Every output was resolved to the arena buffer that contained it when it
        was recorded: a host-side walk over the arenas' buffers, exact whatever the engines allocate afterwards.)"""
        words = torch.cat([t.cpu() for t in self._tables]).tolist() if self._tables else []
        rows = []
        for i, (scope, op, label, buf, dt, r, c) in enumerate(self._meta):
            rows.append(Row.from_words(words[i], seq=i, scope=scope, op=op, output=label, buffer=buf, dtype=dt, rows=r, cols=c))
        return Report(rows)


def _arena_key(p0: int, p1: int) -> str:
    """Name of the live arena buffer that contains bytes [p0, p1), "" for a tensor no engine owns."""
    for arena in list(_ARENAS):
        for key, buf in arena.bufs.items():
            b0 = buf.data_ptr()
            if b0 <= p0 and p1 <= b0 + buf.numel() * buf.element_size():
                return key[0]
    return ""


def record() -> Recorder:
    return Recorder()


def weights(obj) -> Report:
    """The same report over every packed floating-point tensor (f32, f16, e4m3 bytes) of an engine's weights: a bf16 -> f16 /
    e4m3 conversion can over- or underflow too; for fp8 weights the e4m3 bytes and their at_max count are what matter.
    obj: a Seva, AutoEncoder or CLIPConditioner (or an engine); the AutoEncoder contributes its decoder and encoder engines.
    Of a VAE engine's optional packs (e4m3 convs, upsample phase weights) only those it already holds are audited: nothing is
    packed for the report.  E8M0 scale bytes (keys ending in "8e") are no e4m3 numbers and are left out."""
    engines = []
    if hasattr(obj, "encoder_engine"):
        engines = [obj.engine(), obj.encoder_engine()]
    elif hasattr(obj, "engine"):
        engines = [obj.engine()]
    else:
        engines = [obj]
    rec = Recorder()
    seen = set()
    for eng in engines:
        rec.scope = type(eng).__name__
        packs = [eng.W] + [getattr(eng, n) for n in ("W8", "W4") if getattr(eng, n, None) is not None]
        for W in packs:
            for k, t in W.items():
                if not isinstance(t, torch.Tensor) or t.dtype not in DTYPE_NAMES or t.numel() == 0 or k.endswith("8e"):
                    continue
                if (t.data_ptr(), t.dtype) in seen:
                    continue
                seen.add((t.data_ptr(), t.dtype))
                t = t.contiguous()
                cols = t.shape[-1] if t.dim() else 1
                rec.output("weights", k, t, 0, t.numel() // cols, cols, cols)
    rep = rec.report()
    for r in rep.rows:
        r.buffer = ""
    return rep


def check_finite(x: torch.Tensor, what: str = "the final latent") -> None:
    """One `ops.tensor_range` over x and a host sync: raises SevaNativeError if x holds an inf or a NaN.  (SEVA_CHECK_FINITE=1 /
    EulerEDMSampler(check_finite=True) run it after the last step, where `ops.check_handoffs()` syncs anyway.)"""
    t = x if x.dtype in DTYPE_NAMES else x.float()
    w = ops.tensor_range(t.contiguous().view(1, -1))
    n_inf, n_nan = (int(v) for v in w[65:67].tolist())
    if n_inf + n_nan:
        raise _native.SevaNativeError(
            f"{what} holds {n_inf} inf and {n_nan} NaN of {t.numel()} elements: an activation left the f16 / e4m3 range "
            "(frames decoded from it are black).  Rerun with SEVA_AUDIT=<report.json> (or under seva.audit.record()) to see "
            "which launch produced the first non-finite value.")


def check_finite_from_env() -> bool:
    return os.environ.get("SEVA_CHECK_FINITE") == "1"


def merge_into(path: str, key: str, rep: Report) -> None:
    """Merge `rep` into the JSON file at `path` under `key` (the file maps engine class names to reports).  A file that exists
    and is no such JSON object is left as it is: SevaNativeError."""
    data = _merged(path)
    data[key] = rep.to_dict()
    with open(path, "w") as f:
        json.dump(data, f)


def _merged(path: str) -> dict:
    if not os.path.exists(path):
        return {}
    try:
        with open(path) as f:
            data = json.load(f)
    except (OSError, ValueError) as e:
        raise _native.SevaNativeError(f"SEVA_AUDIT: {path} exists and cannot be read as JSON ({e}); move it away, nothing was overwritten") from e
    if not isinstance(data, dict):
        raise _native.SevaNativeError(f"SEVA_AUDIT: {path} exists and holds no report object; move it away, nothing was overwritten")
    return data


def first_call(fn):
    """Entry point of an engine: with SEVA_AUDIT=<path> set, the first call of each engine object runs under a recorder and
    merges its report into the JSON at <path>, keyed by the engine's class; later calls (and every call without the variable)
    run plain.  For programs that cannot be edited to use `record()`."""
    @functools.wraps(fn)
    def wrapper(self, *a, **kw):
        path = os.environ.get("SEVA_AUDIT")
        if not path or getattr(self, "_audit_done", False) or ops._AUDIT is not None or _capturing():
            return fn(self, *a, **kw)
        _merged(path)  # (an unusable file fails here, before the engine runs)
        self._audit_done = True
        with record() as rec:
            out = fn(self, *a, **kw)
        merge_into(path, type(self).__name__, rec.report())
        return out

    return wrapper
