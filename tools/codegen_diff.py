#!/usr/bin/env python3
"""What hipcc emits for the same sources in two trees: per kernel the register / spill / scratch / LDS figures of the compiler's
metadata, instruction counts, whether the instruction stream is identical, and the per-mnemonic counts of the main loop (the
compiler-annotated loop that holds the most MFMAs; ties: the smallest such loop; see loops() for kernels hipcc annotates no loop in)
and of the whole kernel.  Figures and counts only.

    python tools/codegen_diff.py BEFORE_TREE AFTER_TREE gemm.hip conv_win.hip ...     # exit 1 if a figure or a main loop differs

A tree is a checkout root (or a copy of one: stable-virtual-camera_amd/csrc and include/ are enough); files are names under csrc/.
Each file is compiled with its own tree's Makefile flags (CXXFLAGS' code-generation options and FLAGS_<stem>).
"""
import collections
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_lint  # noqa: E402

FIGURES = (("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("vgpr_spill", ".vgpr_spill_count"), ("sgpr_spill", ".sgpr_spill_count"),
           ("private_segment", ".private_segment_fixed_size"), ("lds", ".group_segment_fixed_size"))


def compile_asm(tree, name):
    csrc = os.path.join(tree, "stable-virtual-camera_amd", "csrc")
    try:
        return isa_lint.compile_to_asm(os.path.join(csrc, name), csrc=csrc)
    except RuntimeError as e:
        sys.exit(str(e))


def figures(asm):
    """{kernel symbol: {figure: value}} from the amdhsa.kernels metadata block"""
    out = {}
    for blk in re.split(r"\n  - ", asm[asm.rfind("amdhsa.kernels:"):]):
        sym = re.search(r"\.symbol:\s+'?(\w+)\.kd", blk)
        if sym:
            out[sym.group(1)] = {k: int(re.search(re.escape(key) + r":\s+(\d+)", blk).group(1)) for k, key in FIGURES}
    return out


def loops(asm):
    """{kernel symbol: Counter of the main loop's mnemonics}.  A block belongs to every loop hipcc's annotation names; hipcc annotates
    no loop for irreducible control flow, so where no annotated loop holds an MFMA the loops are the spans of the backward branches
    (target label .. branch), and where no cycle holds one either (fully unrolled) the "loop" is every block that holds an MFMA."""
    out, blocks, cur, member, own = {}, {}, None, set(), None
    for ln in asm.split("\n"):
        m = re.match(r"^(_Z\w+):\s", ln)
        if m:
            cur, member, own = m.group(1), set(), None
            out[cur], blocks[cur] = collections.defaultdict(collections.Counter), [[None, []]]
            continue
        if cur is None:
            continue
        lab = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)(.*)$", ln)
        if lab:
            member = set(re.findall(r"BB\d+_\d+", lab.group(2)))
            if lab.group(1) and "Loop Header" in lab.group(2):
                member.add(lab.group(1))
            own = lab.group(1)
            blocks[cur].append([own, []])
            continue
        cont = re.match(r"^\s+;\s+(Parent Loop|Child Loop|=>This|in Loop)(.*)$", ln)  # the annotation goes on over comment lines
        if cont:
            if cont.group(1) == "Parent Loop":
                member |= set(re.findall(r"BB\d+_\d+", cont.group(2)))
            elif cont.group(1) == "=>This" and own:
                member.add(own)
            continue
        t = ln.split(";")[0].strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            blocks[cur][-1][1].append(t)
            for h in member:
                out[cur][h][t.split(None, 1)[0]] += 1
            if t.startswith("s_endpgm"):
                cur = None
    mfmas = lambda c: sum(v for mn, v in c.items() if "mfma" in mn)  # noqa: E731
    count = lambda bl: collections.Counter(t.split(None, 1)[0] for _, body in bl for t in body)  # noqa: E731

    def best_of(cands):
        best = collections.Counter()
        for c in cands:
            if mfmas(c) > mfmas(best) or (mfmas(c) == mfmas(best) and mfmas(c) > 0 and sum(c.values()) < sum(best.values())):
                best = c
        return best

    main = {}
    for k, pl in out.items():
        best, bl = best_of(pl.values()), blocks[k]
        if mfmas(best) == 0 and mfmas(count(bl)) > 0:
            index = {lab: i for i, (lab, _) in enumerate(bl) if lab}
            spans = []
            for i, (_, body) in enumerate(bl):
                for t in body:
                    tgt = re.search(r"^s_c?branch\w*\s+\.L(BB\d+_\d+)", t)
                    if tgt and index.get(tgt.group(1), i + 1) <= i:
                        spans.append(count(bl[index[tgt.group(1)]:i + 1]))
            best = best_of(spans)
            if mfmas(best) == 0:
                best = count([b for b in bl if any("mfma" in t for t in b[1])])
        main[k] = best
    return main


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not names or not filt:
        return {n: n for n in names}
    res = subprocess.run([filt, *names], capture_output=True, text=True).stdout.split("\n")
    short = [re.sub(r"^(void )?\(anonymous namespace\)::|\(.*$", "", r) for r in res]
    return dict(zip(names, short))


def delta(a, b):
    return {k: (a.get(k, 0), b.get(k, 0)) for k in list(a) + [k for k in b if k not in a] if a.get(k, 0) != b.get(k, 0)}


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    before, after, files = argv[0], argv[1], argv[2:]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        asm = {(t, f): ex.submit(compile_asm, t, f) for t in (before, after) for f in files}
    bad = 0
    for f in files:
        a, b = asm[(before, f)].result(), asm[(after, f)].result()
        ka, kb = isa_lint.kernels(a), isa_lint.kernels(b)
        fa, fb, la, lb = figures(a), figures(b), loops(a), loops(b)
        print(f"== {f}: {len(ka)} kernels before, {len(kb)} after")
        if set(ka) != set(kb):
            print(f"   kernel sets differ: only before {sorted(set(ka) - set(kb))}, only after {sorted(set(kb) - set(ka))}")
            bad += 1
        common = [k for k in ka if k in kb]
        if all(ka[k] == kb[k] and fa.get(k) == fb.get(k) for k in common):
            print("   all identical")
            continue
        names = demangle(common)
        for k in common:
            if ka[k] == kb[k] and fa.get(k) == fb.get(k):
                continue
            regs_eq, loop_eq = fa.get(k) == fb.get(k), la[k] == lb[k]
            bad += (not regs_eq) + (not loop_eq)
            print(f"   {names[k]}")
            print(f"      regs before {fa.get(k)}")
            print(f"      regs after  {fb.get(k)}  {'EQUAL' if regs_eq else 'DIFFERENT'}")
            print(f"      instructions {len(ka[k])} -> {len(kb[k])}; stream {'IDENTICAL' if ka[k] == kb[k] else 'differs'}; main loop "
                  f"{sum(la[k].values())} -> {sum(lb[k].values())} mnemonic counts {'equal' if loop_eq else 'DIFFERENT ' + str(delta(la[k], lb[k]))}")
            mn = lambda body: collections.Counter(t.split(None, 1)[0] for t in body)  # noqa: E731
            if ka[k] != kb[k]:
                print(f"      whole-kernel mnemonic delta: {delta(mn(ka[k]), mn(kb[k]))}")
        same = sum(1 for k in common if ka[k] == kb[k] and fa.get(k) == fb.get(k))
        print(f"   ({same} of {len(common)} kernels identical)")
    print("RESULT: ok (registers and main loops equal)" if not bad else f"RESULT: {bad} differences in registers or main loops")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
