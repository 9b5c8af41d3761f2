"""Closure of tests/kernel_cases.py over the GEMM / conv instantiation tables (csrc/gemm_plan.h), checked without a GPU.

THE RULE: every table row has an exact case.  A new instantiation without a case fails here, and so does a case that names a retired
row, a case whose launch no longer takes the row it names, and a row whose cases have been thinned below the conditions of CONDITIONS.

csrc/gemm_plan_dump.cpp plans every case (`kernel_cases.descriptor`).  tests/test_kernel_coverage_gpu.py launches the same cases
(`kernel_cases.launch`), compares them with an fp64 reference and checks the row through `ops.last_plan()`.
"""
import pytest

import kernel_cases as kc
from conftest import PKG
from test_gemm_plan_cpu import BATCHES, _sweep, conv

pytestmark = pytest.mark.skipif(kc.CXX is None, reason="no g++")

# Rows that no descriptor which validate() accepts can reach: row -> reason.  (None today.  Removing a dead instantiation is a change of
# its own; a row listed here must not be named by any plan of the dispatch sweep of test_gemm_plan_cpu.py.)
UNREACHABLE = {}


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return kc.build_plan_dump(tmp_path_factory.mktemp("kernel_coverage"), PKG)


@pytest.fixture(scope="module")
def rows(dump):
    """name -> table row (its columns as ints, `table`)"""
    return {r["name"]: {k: (v if k in ("table", "name") else int(v)) for k, v in r.items()} for r in dump.tables()}


@pytest.fixture(scope="module")
def planned(dump):
    """[(case, plan)]"""
    return list(zip(kc.CASES, dump([kc.descriptor(c) for c in kc.CASES])))


def test_every_case_takes_the_row_it_names(planned):
    for c, p in planned:
        assert p["kernel"] in ("gemm", "window"), (c.id, p)
        assert p["name"] == c.row, f"{c.id}: planned on '{p['name']}'"
        assert p.get("dbgk", "0") == "0", c.id  # never an ablation twin
        assert c.kind in kc.GEMM_KINDS + kc.CONV_KINDS and c.prec in ("f16", "e4m3") and c.ops <= set(kc.OPERANDS), c.id
        assert ("w_exp" in c.ops) == (c.prec == "e4m3") and ("row_add" in c.ops) == (c.rpg > 0), c.id
        assert all(k in kc.KNOBS for k, _ in c.knobs), c.id


def test_the_rows_of_the_case_list_are_the_rows_of_the_tables(rows):
    have = {c.row for c in kc.CASES}
    want = set(rows) - set(UNREACHABLE)
    assert len(rows) == 81
    assert have == want, f"rows without a case: {sorted(want - have)}; cases that name no row: {sorted(have - want)}"


def test_unreachable_rows_are_not_planned_by_the_sweep(dump, rows):
    assert set(UNREACHABLE) <= set(rows)
    if UNREACHABLE:
        plans = dump([conv(n, *a, **kw) for _, a, kw in _sweep() for n in BATCHES])
        assert not {p.get("name") for p in plans} & set(UNREACHABLE)


def test_launches_stay_small():
    """M N K <= 2 * 10^9 for every case (the largest: the 2-D tiles of the 8-wave e4m3 upsample row, which need 208 output columns)"""
    for c in kc.CASES:
        M, N, K = kc.problem(c)
        assert M * N * K <= 2.0e9, (c.id, M * N * K)


# ------------------------------------------------------------------------------------------------------------------------------------
# what the cases of a row must do together
# ------------------------------------------------------------------------------------------------------------------------------------

def facts(c, p, r):
    """a case as its kernel sees it: rows M, hw pixels per image and ow columns of the image the launch rows index (the phase kernels: the
    SOURCE image), K-tiles of the pipeline, whether a tile of consecutive rows holds pixels of two images"""
    f = dict(case=c, ops=c.ops, n=1, hw=0, ow=0, ih=0, iw=0, stride=c.stride, pad_br=c.pad_br, rpg=c.rpg)
    M, N, K = kc.problem(c)
    kt = K // (128 if c.prec == "e4m3" else 64)
    if c.kind in kc.CONV_KINDS:
        n, ih, iw, cin, _ = c.shape
        oh, ow = kc.conv_geometry(c)[:2]
        if c.kind in ("phases", "phases128"):
            oh, ow, M = ih, iw, n * ih * iw
            kt = cin // 64  # K = 4 cin: the K-tile count is always even; what varies is the number of 64-channel slabs
        f.update(n=n, hw=oh * ow, ow=ow, ih=ih, iw=iw)
    if r.get("splitk"):
        kt //= 2  # per half
    f.update(M=M, N=N, ktiles=kt)
    bm, hw = r["bm"], f["hw"]
    consecutive = p["kernel"] == "gemm" or (p["linear"] == "1" and p["full" if p["n_full"] != "0" else "tail"].split("/")[1] == "0")
    f["straddles"] = bool(hw) and consecutive and any(t * bm < k * hw < min((t + 1) * bm, M) for t in range((M + bm - 1) // bm)
                                                        for k in range(1, f["n"]))
    return f


def _is_conv(r):
    return r["table"] == "win" or r["mode"] != 0


def _two_d(r):
    return r["table"] == "win" and r["tw"] > 0


def _stats_only(r):
    return r["name"] == "win 4-wave 128x160 linear stats"  # chosen only WITH statistics (without: 160 x 160): hw % 64 == 0, so M % 64 == 0


def supported(r):
    """the epilogue operands an instantiation takes"""
    if r["table"] == "win":
        if r["ph"]:
            s = {"bias", "out_f32"}
        else:
            s = {"bias", "row_add", "residual", "out_f32", "out_f16"}
        s |= {"ch_stats"} if r["stats"] else set()
        s |= {"out_f8"} if r["o8"] else set()
        return s | ({"w_exp"} if r["fp8"] else set())
    if r["epi"] == 1:
        s = {"bias", "out_f16"} | (set() if r["astat"] else {"out_f32"}) | ({"out_f8"} if r["fp8"] else set())
    elif r["paired"]:
        s = {"bias", "row_add", "out_f16"}
    else:
        s = {"bias", "row_add", "residual", "out_f32", "out_f16"}
        s |= {"ch_stats"} if r["bm"] == 128 and r["bn"] >= 128 and not r["split16"] else set()  # a wave owns a 64-row block
    s |= {"splitk_ws"} if r["splitk"] else set()
    s |= {"a2"} if r["mode"] == 3 else set()
    return s | ({"w_exp"} if r["fp8"] else set())


def required(r):
    """the operands a row's name requires: never absent"""
    name, s = r["name"], set()
    for token, op in (("f32", "out_f32"), ("f16-only", "out_f16"), ("A-in-regs", "out_f16"), ("split-out", "out_f16"), ("out_f8", "out_f8"),
                      ("e4m3", "w_exp"), ("phases", "out_f32"), ("+ a2", "a2"), ("+ a2", "out_f32"), ("split-K", "splitk_ws")):
        if token in name.split() or (token == "+ a2" and token in name):
            s.add(op)
    if r["bn"] == 32:
        s.discard("out_f32")  # the narrow rows also run the launches with an f16 output only
    return s | ({"ch_stats", "out_f32"} if _stats_only(r) else set())  # (statistics are those of the fp32 output)


# (condition, the rows it applies to, what the facts F of the row's cases must satisfy)
CONDITIONS = [
    ("M: one full tile + a ragged tail that is no multiple of 16",
     lambda r: not _two_d(r) and not _stats_only(r), lambda F, r: any(f["M"] > r["bm"] and f["M"] % r["bm"] % 16 != 0 for f in F)),
    ("M: a tail of half a tile (statistics: M % 64 == 0)", _stats_only, lambda F, r: any(f["M"] > r["bm"] and f["M"] % r["bm"] for f in F)),
    ("M below one tile (2-D tiles are whole tiles)", lambda r: not _two_d(r), lambda F, r: any(f["M"] < r["bm"] for f in F)),
    ("N: a partial last tile (gemm_kernel; 160 split-out columns are chosen by N % 160 == 0)",
     lambda r: r["table"] == "gemm" and r["bn"] >= 128 and not (r["split16"] and r["bn"] == 160), lambda F, r: any(f["N"] % r["bn"] for f in F)),
    ("N < 32 on the narrow rows", lambda r: r["bn"] == 32, lambda F, r: any(f["N"] < 32 for f in F)),
    ("N: more than one tile", lambda r: r["bn"] >= 128, lambda F, r: any(f["N"] > r["bn"] for f in F)),
    ("an odd number of K-tiles (split-K: per half; phases: of 64-channel slabs)", lambda r: True,
     lambda F, r: any(f["ktiles"] % 2 == 1 and (f["ktiles"] >= 3 or r.get("ph")) for f in F)),
    ("an even number of K-tiles (split-K: per half; phases: of 64-channel slabs)", lambda r: True,
     lambda F, r: any(f["ktiles"] % 2 == 0 and (f["ktiles"] >= 4 or r.get("ph")) for f in F)),
    ("conv: an image whose rows do not divide the tile", lambda r: _is_conv(r) and not _two_d(r), lambda F, r: any(f["hw"] % r["bm"] for f in F)),
    ("conv: a tile that straddles two images", lambda r: _is_conv(r) and not _two_d(r), lambda F, r: any(f["straddles"] for f in F)),
    ("conv: at least two images", _is_conv, lambda F, r: any(f["n"] >= 2 for f in F)),
    ("conv: border and interior pixels, every output compared (all four borders of the padding run)", _is_conv,
     lambda F, r: all(f["ih"] >= 3 and f["iw"] >= 3 for f in F)),
    # (the planner takes 2-D tiles only where the tile columns are whole: ow % 16 == 0.  What can vary is their number, and the width of
    # the source image of the upsample / stride-2 rows.)
    ("2-D tiles: an odd number (>= 3) of 16-column tiles per row", _two_d, lambda F, r: any(f["ow"] % 32 == 16 and f["ow"] >= 48 for f in F)),
    ("2-D tiles over an upsampled / strided source: a source width that is no multiple of 16", lambda r: _two_d(r) and (r["up"] or r["s2"]),
     lambda F, r: any(f["iw"] % 16 for f in F)),
    ("2-D tiles: two tile rows in one image", _two_d, lambda F, r: any(f["hw"] // f["ow"] >= 2 * r["bm"] // 16 for f in F)),
    ("stride 2: odd and even input sides", lambda r: r.get("s2"),
     lambda F, r: any(f["ih"] % 2 and f["iw"] % 2 for f in F) and any(f["ih"] % 2 == 0 and f["iw"] % 2 == 0 for f in F)),
    ("the gather: a stride-2 case", lambda r: r["table"] == "gemm" and r["mode"] == 1 and not r["splitk"], lambda F, r: any(f["stride"] == 2 for f in F)),
    ("split-K: at least 2 samples in every case", lambda r: r.get("splitk"), lambda F, r: all(f["n"] >= 2 for f in F)),
    ("every supported operand is present in a case", lambda r: True, lambda F, r: set().union(*(f["ops"] for f in F)) >= supported(r)),
    ("no case names an operand the row does not take", lambda r: True, lambda F, r: set().union(*(f["ops"] for f in F)) <= supported(r)),
    ("out_f32 and out_f16 together", lambda r: {"out_f32", "out_f16"} <= supported(r), lambda F, r: any({"out_f32", "out_f16"} <= f["ops"] for f in F)),
    ("every operand the name does not require is absent in a case", lambda r: True,
     lambda F, r: all(any(o not in f["ops"] for f in F) for o in supported(r) - required(r))),
    ("the operands the name requires are in every case", lambda r: True, lambda F, r: all(required(r) <= f["ops"] for f in F)),
    ("row_add groups that do not divide the tile height", lambda r: "row_add" in supported(r),
     lambda F, r: any(f["rpg"] and r["bm"] % f["rpg"] for f in F)),
]


def test_the_cases_of_a_row_meet_the_conditions(planned, rows):
    by_row = {}
    for c, p in planned:
        by_row.setdefault(c.row, []).append(facts(c, p, rows[c.row]))
    missed = [f"{name}: {what}" for name, F in sorted(by_row.items()) for what, applies, holds in CONDITIONS
              if applies(rows[name]) and not holds(F, rows[name])]
    assert not missed, "\n".join(missed)


def test_the_gather_has_both_paddings_of_stride_2_on_odd_and_even_sides():
    s2 = [c for c in kc.CASES if c.stride == 2 and c.row.startswith("conv gather")]
    for pad_br in (False, True):
        sides = {(c.shape[1] % 2, c.shape[2] % 2) for c in s2 if c.pad_br == pad_br}
        assert {s for side in sides for s in side} == {0, 1}, (pad_br, sides)
