"""The C ABI, checked in one place: include/seva_hip.h against its hand-written restatement in seva/_native.py (every struct, every
prototype, the layout the host compiler gives the structs) and the contract constants against seva/ops.py / seva/_native.py.
The header is parsed once; the comparison functions take the parsed header and the Python objects and return a list of
differences, so that `test_drift_is_detected` can hand them mutated copies.  Only the last test needs the built library."""
import copy
import ctypes as C
import inspect
import os
import re
import subprocess
import types

import pytest
import torch

from conftest import ROOT
from kernel_cases import CXX
from seva import _native, ops

HEADER = os.path.join(ROOT, "include", "seva_hip.h")

# ---- the explicit type map ------------------------------------------------------------------------------------------------
SCALARS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "int": C.c_int, "double": C.c_double,
           "uint8_t": C.c_uint8, "uint64_t": C.c_uint64}

# header macro / enumerator -> (the Python name that restates it, its value)
CONSTANTS = {
    "SEVA_ABI_VERSION": ("_native.ABI_VERSION", _native.ABI_VERSION),
    "SEVA_PROF_CLASSES": ("_native.PROF_CLASSES", _native.PROF_CLASSES),
    "SEVA_CH_STATS_ROWS": ("ops.STATS_ROWS", ops.STATS_ROWS),
    "SEVA_SPLITK_FLAGS": ("ops.SPLITK_FLAGS", ops.SPLITK_FLAGS),
    "SEVA_SPLITK_ERROR_SLOT": ("ops.SPLITK_ERROR_SLOT", ops.SPLITK_ERROR_SLOT),
    "SEVA_SPLITK_TILE_M": ("ops.SPLITK_TILE_M", ops.SPLITK_TILE_M),
    "SEVA_SPLITK_TILE_N": ("ops.SPLITK_TILE_N", ops.SPLITK_TILE_N),
    "SEVA_SPLITK_MAX_PIXELS": ("ops.SPLITK_MAX_PIXELS", ops.SPLITK_MAX_PIXELS),
    "SEVA_ATTN_LONG_MIN_LQ": ("ops.PV8_MIN_LQ", ops.PV8_MIN_LQ),
    "SEVA_ATTN_SPLIT_MIN_LK": ("ops.ATTN_SPLIT_MIN_LK", ops.ATTN_SPLIT_MIN_LK),
    "SEVA_ATTN_SPLIT_ROW_FLOATS": ("ops.ATTN_SPLIT_ROW_FLOATS", ops.ATTN_SPLIT_ROW_FLOATS),
    "SEVA_GN_WORKSPACE_SLABS": ("ops.GN_WORKSPACE_SLABS", ops.GN_WORKSPACE_SLABS),
    "SEVA_RANGE_WORDS": ("ops.RANGE_WORDS", ops.RANGE_WORDS),
    "SEVA_RANGE_WG_ELEMS": ("ops.RANGE_WG_ELEMS", ops.RANGE_WG_ELEMS),
    "SEVA_RANGE_MAX_WGS": ("ops.RANGE_MAX_WGS", ops.RANGE_MAX_WGS),
    "SEVA_RANGE_F32": ("ops.RANGE_DTYPES[float32]", ops.RANGE_DTYPES[torch.float32]),
    "SEVA_RANGE_F16": ("ops.RANGE_DTYPES[float16]", ops.RANGE_DTYPES[torch.float16]),
    "SEVA_RANGE_E4M3": ("ops.RANGE_DTYPES[uint8]", ops.RANGE_DTYPES[torch.uint8]),
}
# header constants with no Python counterpart, and why
C_ONLY = {
    "SEVA_OK": "the binding tests rc != 0 and raises with seva_last_error(); no code is named",
    "SEVA_ERR_ARG": "as SEVA_OK",
    "SEVA_ERR_LAUNCH": "as SEVA_OK",
    "SEVA_ERR_UNSUPPORTED": "as SEVA_OK",
}


# ---- the header, parsed -----------------------------------------------------------------------------------------------------
def _norm(ctype: str) -> str:
    """'const float *' -> 'float*'"""
    return re.sub(r"\s+", "", re.sub(r"\bconst\b", "", ctype))


def _declarators(decl: str):
    """'int64_t M, N, K' -> ('int64_t', ['M', 'N', 'K']); 'const void* a' -> ('void*', ['a'])"""
    m = re.fullmatch(r"(.*?[\s*])([A-Za-z_]\w*(?:\s*,\s*[A-Za-z_]\w*)*)", decl.strip(), re.S)
    assert m, f"cannot parse declaration {decl!r}"
    return _norm(m.group(1)), re.split(r"\s*,\s*", m.group(2))


def parse_header(text: str) -> types.SimpleNamespace:
    """structs: {name: [(field, C type)]} in declaration order; protos: {name: (return type, [argument types])}; consts: {name: int}
    of every integer `#define SEVA_*` and enumerator.  Types are normalised ('float*'), typedefs of the header resolved."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    consts = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(SEVA_\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M):
        m = re.fullmatch(r"\(?\s*(-?\d+)\s*\)?", value)
        assert m, f"#define {name} {value}: not an integer literal (write the number out: the Python side restates a number)"
        consts[name] = int(m.group(1))
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)  # preprocessor lines
    for body in re.findall(r"\benum\s*\{(.*?)\}\s*;", text, re.S):
        for name, value in re.findall(r"(\w+)\s*=\s*(-?\d+)", body):
            consts[name] = int(value)
    text = re.sub(r"\benum\s*\{.*?\}\s*;", "", text, flags=re.S)
    structs = {}
    for name, body, alias in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text, re.S):
        assert name == alias, (name, alias)
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            ctype, names = _declarators(decl)
            fields += [(n, ctype) for n in names]
        structs[name] = fields
    text = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    typedefs = {}
    for ctype, name in re.findall(r"typedef\s+([^;{}]+?[\s*])(\w+)\s*;", text):
        typedefs[name] = _norm(ctype)
    text = re.sub(r"typedef\s+[^;{}]+;", "", text)
    text = re.sub(r'extern\s+"C"\s*\{', "", text)
    resolve = lambda t: typedefs.get(t, t)  # noqa: E731
    protos = {}
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        if stmt == "}":  # the closing brace of extern "C"
            continue
        m = re.fullmatch(r"(.*?[\s*])(\w+)\s*\((.*)\)", stmt, re.S)
        assert m, f"cannot parse {stmt!r}"
        args = []
        if m.group(3).strip() != "void":
            for p in m.group(3).split(","):
                pm = re.fullmatch(r"(.*?[\s*])(\w+)", p.strip(), re.S)  # every parameter of the header is named
                assert pm, f"{m.group(2)}: cannot parse parameter {p!r}"
                args.append(resolve(_norm(pm.group(1))))
        protos[m.group(2)] = (resolve(_norm(m.group(1))), args)
    return types.SimpleNamespace(structs=structs, protos=protos, consts=consts)


@pytest.fixture(scope="module")
def hdr():
    with open(HEADER) as f:
        return parse_header(f.read())


def binding_structs() -> dict:
    """{class name: (class, [(field, ctype)])} of every ctypes.Structure of seva/_native.py"""
    return {n: (c, list(c._fields_)) for n, c in vars(_native).items()
            if inspect.isclass(c) and issubclass(c, C.Structure) and c.__module__ == _native.__name__}


def class_of(struct: str, classes: dict):
    """seva_lpips_layer_desc -> LpipsLayerDesc: the prefix dropped, underscores and case ignored; None if there is none or several"""
    key = struct.replace("seva_", "", 1).replace("_", "").lower()
    hits = [n for n in classes if n.lower() == key]
    return hits[0] if len(hits) == 1 else None


# ---- the comparisons: each returns a list of differences, [] = equal ---------------------------------------------------------
def struct_field_ctype(ctype: str):
    return C.c_void_p if ctype.endswith("*") else SCALARS[ctype]


def diff_structs(h, classes: dict) -> list:
    out, used = [], set()
    for struct, fields in h.structs.items():
        cls = class_of(struct, classes)
        if cls is None:
            out.append(f"{struct}: not exactly one Structure in _native.py")
            continue
        used.add(cls)
        py = classes[cls][1]
        if [n for n, _ in fields] != [n for n, _ in py]:
            k = next((i for i, (a, b) in enumerate(zip(fields, py)) if a[0] != b[0]), min(len(fields), len(py)))
            out.append(f"{struct} / {cls}: field names differ from position {k}: header {[n for n, _ in fields][k:k + 3]}, "
                       f"binding {[n for n, _ in py][k:k + 3]}")
            continue
        out += [f"{struct}.{n}: header {ct}, binding {pt.__name__} (expected {struct_field_ctype(ct).__name__})"
                for (n, ct), (_, pt) in zip(fields, py) if pt is not struct_field_ctype(ct)]
    out += [f"{cls}: a Structure of _native.py with no struct in the header" for cls in classes if cls not in used]
    return out


def arg_ctypes(ctype: str, h, classes: dict) -> tuple:
    """the ctypes an argument (or return value) of this C type may be bound as"""
    if not ctype.endswith("*"):
        return (SCALARS[ctype],)
    base = ctype[:-1]
    if base in h.structs:
        cls = class_of(base, classes)
        return (C.POINTER(classes[cls][0]),) if cls else ()
    if base == "char":
        return (C.c_char_p,)
    if base == "void*":
        return (C.POINTER(C.c_void_p),)
    if base == "void":
        return (C.c_void_p,)
    return (C.c_void_p, C.POINTER(SCALARS[base]))


def _tn(t) -> str:
    return getattr(t, "__name__", repr(t))


def diff_protos(h, symbols: dict, classes: dict) -> list:
    out = [f"declared in the header, not in SYMBOLS: {n}" for n in sorted(set(h.protos) - set(symbols))]
    out += [f"in SYMBOLS, not declared in the header: {n}" for n in sorted(set(symbols) - set(h.protos))]
    for name in sorted(set(h.protos) & set(symbols)):
        (ret, args), (res, argtypes) = h.protos[name], symbols[name]
        if res not in arg_ctypes(ret, h, classes):
            out.append(f"{name}: returns {ret}, restype {_tn(res)}")
        if len(args) != len(argtypes):
            out.append(f"{name}: {len(args)} parameters in the header, {len(argtypes)} argtypes")
            continue
        out += [f"{name}: argument {i} is {ct} in the header, {_tn(pt)} in argtypes (expected {' or '.join(map(_tn, arg_ctypes(ct, h, classes)))})"
                for i, (ct, pt) in enumerate(zip(args, argtypes)) if pt not in arg_ctypes(ct, h, classes)]
    return out


def diff_consts(h, table: dict, c_only: dict) -> list:
    out = [f"{n} = {v} of the header is neither in CONSTANTS nor in C_ONLY" for n, v in h.consts.items() if n not in table and n not in c_only]
    out += [f"{n}: in CONSTANTS / C_ONLY, not an integer constant of the header" for n in list(table) + list(c_only) if n not in h.consts]
    out += [f"{n} = {h.consts[n]} in the header, {py} = {v}" for n, (py, v) in table.items() if n in h.consts and h.consts[n] != v]
    return out


def diff_layout(h, classes: dict, measured: dict) -> list:
    """measured: {'struct' or 'struct.field': sizeof / offsetof as the host compiler sees the header}"""
    out = []
    for struct, fields in h.structs.items():
        cls = classes[class_of(struct, classes)][0]
        if measured[struct] != C.sizeof(cls):
            out.append(f"sizeof({struct}) = {measured[struct]}, ctypes.sizeof({cls.__name__}) = {C.sizeof(cls)}")
        out += [f"offsetof({struct}, {n}) = {measured[f'{struct}.{n}']}, {cls.__name__}.{n}.offset = {getattr(cls, n).offset}"
                for n, _ in fields if measured[f"{struct}.{n}"] != getattr(cls, n).offset]
    return out


# ---- the tests ------------------------------------------------------------------------------------------------------------------
def test_structs_match_the_header(hdr):
    assert len(hdr.structs) >= 8
    diffs = diff_structs(hdr, binding_structs())
    assert not diffs, "\n".join(diffs)


def test_prototypes_match_the_header(hdr):
    assert set(hdr.protos) == set(_native.SYMBOLS), set(hdr.protos) ^ set(_native.SYMBOLS)
    diffs = diff_protos(hdr, _native.SYMBOLS, binding_structs())
    assert not diffs, "\n".join(diffs)


def test_constants_match_the_header(hdr):
    diffs = diff_consts(hdr, CONSTANTS, C_ONLY)
    assert not diffs, "\n".join(diffs)
    assert len(_native.PROF_NAMES) == _native.PROF_CLASSES


def test_abi_version(hdr):
    assert hdr.consts["SEVA_ABI_VERSION"] == _native.ABI_VERSION == 12  # the one place that pins the number


@pytest.mark.skipif(CXX is None, reason="no g++")
def test_struct_layout_matches_the_host_compiler(hdr, tmp_path):
    classes = binding_structs()
    assert not diff_structs(hdr, classes)  # (the names below come from the header: its own test says what differs)
    lines = [f'  printf("{s} %zu\\n", sizeof({s}));' for s in hdr.structs]
    lines += [f'  printf("{s}.{n} %zu\\n", offsetof({s}, {n}));' for s, fields in hdr.structs.items() for n, _ in fields]
    src, exe = tmp_path / "abi_layout.cpp", tmp_path / "abi_layout"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "seva_hip.h"\nint main() {\n' + "\n".join(lines) + "\n  return 0;\n}\n")
    subprocess.run([CXX, "-std=c++17", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    measured = {k: int(v) for k, v in (ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert len(measured) == len(lines)
    diffs = diff_layout(hdr, classes, measured)
    assert not diffs, "\n".join(diffs)


def test_drift_is_detected(hdr):
    """Each comparison reports a planted difference and names the culprit (in memory: no file, no subprocess)."""
    classes = binding_structs()

    def with_fields(cls, fields):
        return {**classes, cls: (classes[cls][0], fields)}

    gemm = classes["GemmDesc"][1]
    i, j = [n for n, _ in gemm].index("lda"), [n for n, _ in gemm].index("ldr")
    swapped = list(gemm)
    swapped[i], swapped[j] = swapped[j], swapped[i]
    d = diff_structs(hdr, with_fields("GemmDesc", swapped))
    assert len(d) == 1 and "seva_gemm_desc" in d[0] and "'lda'" in d[0] and "'ldr'" in d[0], d

    widened = [(n, C.c_int64 if n == "lq" else t) for n, t in classes["AttnDesc"][1]]
    d = diff_structs(hdr, with_fields("AttnDesc", widened))
    assert d == [f"seva_attn_desc.lq: header int32_t, binding {C.c_int64.__name__} (expected {C.c_int32.__name__})"], d

    symbols = copy.copy(_native.SYMBOLS)
    res, args = symbols["seva_cfg_multistep_f32"]
    symbols["seva_cfg_multistep_f32"] = (res, args[:-1])
    d = diff_protos(hdr, symbols, classes)
    assert d == ["seva_cfg_multistep_f32: 12 parameters in the header, 11 argtypes"], d

    symbols = copy.copy(_native.SYMBOLS)
    symbols["seva_gemm_fp8"] = (C.c_int, [C.POINTER(_native.AttnDesc), C.c_void_p])
    d = diff_protos(hdr, symbols, classes)
    assert len(d) == 1 and d[0].startswith("seva_gemm_fp8: argument 0 is seva_gemm_desc*") and "LP_AttnDesc" in d[0] and "LP_GemmDesc" in d[0], d

    symbols = copy.copy(_native.SYMBOLS)
    symbols["seva_attn_v_fp8_size"] = (C.c_int, [C.c_int32] * 3 + [C.POINTER(C.c_int32), C.POINTER(C.c_int64)])  # T* bound as another T
    del symbols["seva_last_plan"]
    d = diff_protos(hdr, symbols, classes)
    assert len(d) == 2 and "seva_last_plan" in d[0] and d[1].startswith("seva_attn_v_fp8_size: argument 3 is int64_t*"), d

    table = {**CONSTANTS, "SEVA_ATTN_SPLIT_MIN_LK": ("ops.ATTN_SPLIT_MIN_LK", ops.ATTN_SPLIT_MIN_LK + 1)}
    d = diff_consts(hdr, table, C_ONLY)
    assert d == ["SEVA_ATTN_SPLIT_MIN_LK = 6144 in the header, ops.ATTN_SPLIT_MIN_LK = 6145"], d
    moved = types.SimpleNamespace(consts={**hdr.consts, "SEVA_SPLITK_FLAGS": hdr.consts["SEVA_SPLITK_FLAGS"] - 1, "SEVA_NEW_LIMIT": 7})
    d = diff_consts(moved, CONSTANTS, C_ONLY)
    assert len(d) == 2 and "SEVA_NEW_LIMIT = 7" in d[0] and d[1].startswith("SEVA_SPLITK_FLAGS = 16383 in the header, ops.SPLITK_FLAGS = 16384"), d

    measured = {s: C.sizeof(classes[class_of(s, classes)][0]) for s in hdr.structs}
    measured.update({f"{s}.{n}": getattr(classes[class_of(s, classes)][0], n).offset for s, fields in hdr.structs.items() for n, _ in fields})
    assert not diff_layout(hdr, classes, measured)
    measured["seva_range_desc.rows"] -= 4  # what a packed struct would give
    d = diff_layout(hdr, classes, measured)
    assert d == ["offsetof(seva_range_desc, rows) = 12, RangeDesc.rows.offset = 16"], d


def test_library_exports_every_declared_symbol(hdr):
    """The built library against the header (needs no GPU: nothing is launched)."""
    lib = C.CDLL(_native.LIB_PATH)
    missing = [name for name in hdr.protos if not hasattr(lib, name)]
    assert not missing, missing
    assert _native.load().seva_abi_version() == hdr.consts["SEVA_ABI_VERSION"]
