"""The A/B variant of the library (`make variant NAME=x EXTRA=...`, csrc/Makefile) is built like the shipped one: every source's
compile line carries the options of the shipped object's line, the file's own FLAGS_<stem> among them, plus EXTRA.  A file whose flags
were missing from the variant would give an A/B library that measures something nobody ships.  Only `make -n` runs: no compiler."""
import os
import subprocess
import sys

from conftest import PKG, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_lint  # noqa: E402  (production_sources, file_flags: the Makefile's SRCS and FLAGS_<stem>)


def _compile_lines(*args):
    """{source: (options, output)} of the compile lines `make -n ARGS` prints"""
    out = subprocess.run(["make", "-n", "-C", os.path.join(PKG, "csrc"), *args], check=True, capture_output=True, text=True).stdout
    lines = {}
    for words in (ln.split() for ln in out.split("\n") if " -c " in ln):
        src, obj = words[words.index("-c") + 1], words[words.index("-o") + 1]
        assert src not in lines, (src, "compiled twice")
        lines[src] = ([w for w in words[1:] if w not in ("-c", src, "-o", obj)], obj)
    return lines


def test_variant_objects_are_built_like_the_shipped_ones():
    srcs = [os.path.basename(s) for s in isa_lint.production_sources()]
    shipped, variant = _compile_lines("-B", "all"), _compile_lines("variant", "NAME=t", "EXTRA=-DX")
    assert sorted(shipped) == sorted(variant) == sorted(srcs)
    for src in srcs:
        (opts, obj), (vopts, vobj) = shipped[src], variant[src]
        assert obj == src[:-4] + ".o" and vobj.endswith("build_ab/obj_t/" + obj), (src, obj, vobj)
        assert "-DX" not in opts and vopts.count("-DX") == 1 and [w for w in vopts if w != "-DX"] == opts, (src, opts, vopts)
        own = isa_lint.file_flags(src)
        assert opts[len(opts) - len(own):] == own, (src, opts, own)  # the file's own flags did reach both lines
