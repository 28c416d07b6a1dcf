#!/usr/bin/env python3
"""Code bytes of one kernel and of its loops, from the compiler's own assembly (hipcc -save-temps=obj keeps it).

The file is assembled again with llvm-mc, local labels kept (-save-temp-labels), and the label addresses are read back from
the object's symbol table: the kernel's size, the address range of every loop tools/isa_loops.py lists (a backward branch to
a label; body = label .. branch), and the address of every s_barrier -- a fetch after a barrier starts at that cache line
(64 B).  Addresses are relative to the kernel's first instruction.

    python tools/isa_bytes.py <file.s> '<demangled-name substring>' [--min BYTES]
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def main():
    path, want = sys.argv[1], sys.argv[2]
    minb = int(sys.argv[sys.argv.index("--min") + 1]) if "--min" in sys.argv else 256
    src = open(path).read().split("\n")
    # a label in front of every s_barrier, so that its address lands in the symbol table too
    out, nbar = [], 0
    for ln in src:
        if re.match(r"^\ts_barrier\b", ln):
            out.append(".Lisa_bytes_bar_%d:" % nbar)
            nbar += 1
        out.append(ln)
    with tempfile.TemporaryDirectory() as tmp:
        s, o = os.path.join(tmp, "a.s"), os.path.join(tmp, "a.o")
        open(s, "w").write("\n".join(out))
        subprocess.check_call([os.path.join(LLVM, "llvm-mc"), "-triple=amdgcn-amd-amdhsa", "-mcpu=gfx950", "-filetype=obj",
                               "-save-temp-labels", "-o", o, s])
        syms = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-t", o], capture_output=True, text=True, check=True).stdout
    addr, size = {}, {}
    for ln in syms.split("\n"):
        f = ln.split()
        sec = [i for i, x in enumerate(f) if x.startswith(".text")]                # (a section per function; `.protected` may follow the size)
        if len(f) >= 4 and re.fullmatch(r"[0-9a-f]{16}", f[0]) and sec and sec[0] + 2 < len(f) + 1:
            addr[f[-1]] = int(f[0], 16)
            size[f[-1]] = int(f[sec[0] + 1], 16)
    cur, funcs = None, {}
    for ln in out:
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur = m.group(1)
            funcs[cur] = []
        elif ln.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            funcs[cur].append(ln)
    for name, lines in funcs.items():
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        if want not in dem:
            continue
        base = addr[name]
        print(dem)
        print("kernel: %d bytes (%d lines of 64 B)" % (size[name], (size[name] + 63) // 64))
        seen, pos, loops, bars, last = {}, 0, [], [], None
        for ln in lines:
            m = re.match(r"^(\.L\w+):", ln)
            if m:
                seen[m.group(1)] = pos
                last = m.group(1)
                if last.startswith(".Lisa_bytes_bar_"):
                    bars.append(addr[last] - base)
                continue
            if ln.startswith("\t") and ln.strip() and not ln.lstrip().startswith((".", ";")):
                tok = ln.split()
                pos += 1
                if tok[0].startswith(("s_cbranch", "s_branch")) and len(tok) > 1 and tok[1] in seen and tok[1].startswith(".LBB"):
                    loops.append((addr[tok[1]] - base, tok[1], pos - seen[tok[1]], last))
        print("%-12s %8s %8s %8s" % ("loop", "start", "insts", "bytes>="))
        for a, lab, n, lastlab in sorted(loops):
            end = addr[lastlab] - base            # the last label ahead of the branch: a lower bound of the body's end
            if end - a >= minb:
                print("%-12s %8d %8d %8d" % (lab, a, n, end - a))
        print("s_barrier at (byte, offset within its 64 B line): " + " ".join("%d+%d" % (b // 64 * 64, b % 64) for b in bars))


if __name__ == "__main__":
    main()
