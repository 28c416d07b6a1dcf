#!/usr/bin/env python3
"""Is the device code of two builds the same?  A text comparison of the compiler's own assembly.

`make -C hmc.jl_amd/csrc` keeps, beside every object, the device assembly of its translation unit
(obj/<unit>-hip-amdgcn-amd-amdhsa-gfx950.s).  Given two such object directories this tool compares every
unit present in either, after a normalisation that removes only what cannot reach the GPU:

  * comments (a `;` and everything behind it) and trailing blanks,
  * `.file`, `.loc`, `.cfi*` and `.ident` lines.

Labels, the `.amdhsa_*` kernel descriptors and the `.amdgpu_metadata` block (register and spill counts) stay in.
One line per unit, `identical` or `differs`; under a unit that differs, the kernels that differ (each file is cut
at its `.globl` / `.type ...,@function` / `.type ...,@object` lines and at the kernel entries of the metadata block).  Exit status 1 if
anything differs or a unit exists on one side only.  A refactor of always-inlined kernel code is done when this
prints `identical` for every unit against the parent commit's build.

    python3 tools/isa_same.py <parent>/hmc.jl_amd/csrc/obj hmc.jl_amd/csrc/obj
"""
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_lint import demangle_short  # noqa: E402

SUFFIX = re.compile(r"^(.*)-hip-amdgcn-amd-amdhsa-gfx\w+\.s$")
SKIP = re.compile(r"^\s*\.(file|loc|cfi\w*|ident)\b")
GLOBL = re.compile(r"^\s*\.globl\s+(\S+)")
SYMBOL = re.compile(r"^\s*\.type\s+([^\s,]+),@(function|object)")
META_KERNEL = re.compile(r"^  - \.")              # an entry of the metadata's amdhsa.kernels list
META_NAME = re.compile(r"^    \.name:\s+(\S+)")


def normalise(text):
    out = []
    for raw in text.splitlines():
        line = raw.split(";", 1)[0].rstrip()
        if line and not SKIP.match(line):
            out.append(line)
    return out


def pieces(lines):
    """{symbol: [lines]} in file order; what precedes the first symbol is filed under ''."""
    out, cur, in_meta = {}, "", False
    for n, line in enumerate(lines):
        s = line.strip()
        if s == ".amdgpu_metadata":
            in_meta, cur = True, ""
        elif s == ".end_amdgpu_metadata":
            in_meta, cur = False, ""
        elif in_meta:
            if META_KERNEL.match(line):
                cur = ""
                for later in lines[n + 1:]:
                    if META_KERNEL.match(later) or not later.startswith("    "):
                        break
                    m = META_NAME.match(later)
                    if m:
                        cur = m.group(1)
                        break
        else:
            m = GLOBL.match(line) or SYMBOL.match(line)
            if m:
                cur = m.group(1)
        out.setdefault(cur, []).append(line)
    return out


def differing(a_text, b_text):
    """Names of the pieces that differ between two assembly texts (empty list: the same)."""
    a, b = pieces(normalise(a_text)), pieces(normalise(b_text))
    return [demangle_short(k) if k else "(outside any symbol)" for k in list(a) + [k for k in b if k not in a] if a.get(k) != b.get(k)]


def units(objdir):
    found = {}
    for p in glob.glob(os.path.join(objdir, "*.s")):
        m = SUFFIX.match(os.path.basename(p))
        if m:
            found[m.group(1)] = p
    return found


def main(argv):
    if len(argv) != 2:
        print(__doc__)
        return 2
    a, b = units(argv[0]), units(argv[1])
    if not a and not b:
        print("isa_same: no device assembly under %s or %s (build with `make -C hmc.jl_amd/csrc`)" % tuple(argv))
        return 2
    bad = 0
    for u in sorted(set(a) | set(b)):
        if u not in a or u not in b:
            bad += 1
            print("%-22s missing in %s" % (u, argv[0] if u not in a else argv[1]))
            continue
        with open(a[u]) as fa, open(b[u]) as fb:
            diff = differing(fa.read(), fb.read())
        print("%-22s %s" % (u, "differs" if diff else "identical"))
        for k in diff:
            print("    %s" % k)
        bad += 1 if diff else 0
    print("isa_same: %d unit(s), %d not identical" % (len(set(a) | set(b)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
