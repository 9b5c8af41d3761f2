"""Build-time check of attn16_kernel (csrc/attention.hip) on the emitted ISA: the softmax row sums are taken on the matrix pipe
(two v_mfma_f32_16x16x32_f16 per query block against an A fragment of ones: 72 MFMAs per 64 x 64 tile, not 64) and the
v_dot2_f32_f16 chains are gone, while both instantiations stay at two workgroups per CU: at most 256 registers, no scratch.
(hipcc cross-compiles for gfx950 without a GPU; ~20 s.)"""
import os
import re
import sys

import pytest

from conftest import PKG, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_lint  # noqa: E402  (tools/isa_lint.py: the library's compile line)

NAMES = {"unsplit": "_ZN12_GLOBAL__N_113attn16_kernelILi64ELb0EEEvNS_8AttnArgsE",
         "split": "_ZN12_GLOBAL__N_113attn16_kernelILi64ELb1EEEvNS_8AttnArgsE"}


@pytest.fixture(scope="module")
def asm():
    if not os.path.exists(isa_lint.HIPCC):
        pytest.skip("no hipcc")
    return isa_lint.compile_to_asm(os.path.join(PKG, "csrc", "attention.hip"))


def _body(asm, name):
    """every instruction of the function, the blocks the compiler placed behind the first s_endpgm included"""
    m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), asm, re.S | re.M)
    assert m, f"{name} not in the assembly"
    lines = (ln.split(";")[0].strip() for ln in m.group(1).split("\n"))
    return [t for t in lines if t and (not t.startswith(".") or t.startswith(".LBB"))]  # instructions and block labels


def _meta(asm, name):
    m = re.search(r"^  - \.agpr_count:\s+(\d+)\n(?:(?!^  - ).*\n)*?\s+\.name:\s+%s\n(?:(?!^  - ).*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n"
                  r"(?:(?!^  - ).*\n)*?\s+\.vgpr_count:\s+(\d+)\n" % re.escape(name), asm, re.M)
    assert m, f"no metadata of {name}"
    return {"agpr": int(m.group(1)), "private": int(m.group(2)), "vgpr": int(m.group(3))}


@pytest.mark.parametrize("which", sorted(NAMES))
def test_two_workgroups_per_cu(asm, which):
    meta = _meta(asm, NAMES[which])
    print(which, meta)
    assert meta["private"] == 0, meta
    assert meta["vgpr"] + meta["agpr"] <= 256, meta


@pytest.mark.parametrize("which", sorted(NAMES))
def test_row_sums_on_the_matrix_pipe(asm, which):
    body = _body(asm, NAMES[which])
    ops = [t.split()[0] for t in body]
    # (the row sums were v_dot2_f32_f16 in its accumulating encoding, which hipcc prints as v_dot2c_f32_f16_e32: any v_dot2* counts)
    assert not any(o.startswith("v_dot2") for o in ops), which
    assert not any(o.startswith("scratch_") for o in ops), which
    n = sum(o == "v_mfma_f32_16x16x32_f16" for o in ops)
    print(which, "MFMAs in the body:", n)
    assert n >= 72, (which, n)
    # the unmasked steady-state tile is the one loop of the body: from the loop header to the last backward branch to it, its 72 MFMAs
    # (32 scores, 8 row sums, 32 P.V) stand in the blocks that are not the rare path; over the whole loop the count is at least that
    labels = {t[:-1]: i for i, t in enumerate(body) if re.fullmatch(r"\.LBB\d+_\d+:", t)}
    back = [(labels[t.split()[1]], i) for i, t in enumerate(body)
            if t.startswith("s_cbranch") and t.split()[1] in labels and labels[t.split()[1]] < i]
    loops = [sum(body[j].startswith("v_mfma_f32_16x16x32_f16") for j in range(a, b)) for a, b in back]
    assert loops and max(loops) >= 72, (which, loops)
