#!/usr/bin/env python3
"""Hazard check for the inline assembly of libhmcgibbs (run on the compiler's own assembly, csrc/obj/*.s).

The compiler inserts the wait states that gfx950 requires between dependent instructions, but it does not look inside an
asm statement: a hazard whose producer or consumer lies in an `;;#ASMSTART ... ;;#ASMEND` region is the statement's own
business (both assembly bugs of round 4 were of this kind).  This tool finds every such pair.

What it checks: for every instruction that can be the consumer of a rule below, it walks BACK over every path of the
kernel's control flow (fall-through, each branch to a label, loop back-edges, the s_getpc / s_setpc long jumps) and finds
the nearest producer on each path.  The distance is the number of wait states strictly between the two: `s_nop N` counts
N + 1, any other instruction 1.  A pair closer than the rule's count is a finding when the producer or the consumer lies in
an asm region.  Like the compiler, the walk does not stop at a later non-VALU write of the register (an SALU write after
the VALU one, say): it looks for the nearest VALU write.  At the entry of the consumer's region, an unknown VALU
instruction is assumed to have written every register the region reads before writing it (the statement cannot know
what the compiler put in front of it); what the compiler put behind a region is read as it stands.

Rules (gfx940 / gfx950; each count read off hipcc --offload-arch=gfx950 -S on a probe kernel that makes the compiler emit
the pair, unless marked otherwise):
  valu-sgpr>valu       VALU writes an SGPR / VCC -> a VALU reads it (operand, carry-in, v_cndmask mask)       2
                       (v_cmp vcc; s_nop 1; v_cndmask vcc -- and v_readfirstlane s0; s_mul s0; s_nop 0; v_add3 s0)
  valu-sgpr>vmem       VALU writes an SGPR -> a VMEM instruction uses it (saddr, soffset, descriptor)          5
                       (v_readfirstlane s0; s_nop 4; global_load v0, v2, s[0:1])
  valu-sgpr>lanesel    VALU writes an SGPR / VCC -> v_readlane / v_writelane lane select                       4
                       (v_readfirstlane s0; s_nop 3; v_readlane s0, v1, s0)
  valu-vcc>div_fmas    VALU writes VCC -> v_div_fmas (implicit VCC read)                                        4
                       (documented value: the compiler always schedules the pair far apart, no probe reaches it)
  valu-vgpr>dpp        VALU writes a VGPR -> a DPP instruction reads it                                         2
                       (v_lshl_add_u32 v1; s_nop 1; v_mov_b32_dpp v2, v1 row_shr:1)
  valu-exec>dpp        VALU writes EXEC -> any DPP instruction                                                   5
                       (documented value: no probe makes the compiler write EXEC with a VALU instruction)
  valu-vgpr>readlane   VALU writes a VGPR -> v_readfirstlane / v_readlane reads it                              1
                       (v_lshl_add_u64 v[2:3]; s_nop 0; v_readfirstlane s1, v3)
  valu-vgpr>permlane   VALU writes a VGPR -> v_permlane* reads it                                               2
                       (v_add_u32 v2; s_nop 1; v_permlane32_swap v1, v2)
  trans>valu           v_rcp* / v_rsq* / v_sqrt* / v_exp* / v_log* / v_sin* / v_cos* result -> a VALU reads it   1
                       (v_rcp_f64 v[0:1]; s_nop 0; v_add_f64 v[0:1], v[0:1], 1.0)

--outside applies the same table to the compiler's own code only (pairs with both ends outside every asm region): the
compiler pads its code correctly, so any finding there means the table or the walk is wrong (tests/test_asm_hazards.py).

Exit status 1 when there is a finding.
"""
import glob
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OBJ = os.path.join(os.path.dirname(HERE), "hmc.jl_amd", "csrc", "obj")

# rule -> (producer kind, wait states)
RULES = {
    "valu-sgpr>valu": ("sgpr", 2),
    "valu-sgpr>vmem": ("sgpr", 5),
    "valu-sgpr>lanesel": ("sgpr", 4),
    "valu-vcc>div_fmas": ("sgpr", 4),
    "valu-vgpr>dpp": ("vgpr", 2),
    "valu-exec>dpp": ("exec", 5),
    "valu-vgpr>readlane": ("vgpr", 1),
    "valu-vgpr>permlane": ("vgpr", 2),
    "trans>valu": ("trans", 1),
}

KERNEL_START = re.compile(r"^([_A-Za-z][\w$.]*):")
LABEL = re.compile(r"^\s*(\.L[\w$.]*|[_A-Za-z][\w$.]*):")
TRANS = re.compile(r"^v_(rcp|rsq|sqrt|exp|log|sin|cos)(_|$)")
TWO_DEFS = re.compile(r"^v_(add_co|addc_co|sub_co|subb_co|subrev_co|subbrev_co|div_scale|mad_u64_u32|mad_i64_i32)")
VMEM = re.compile(r"^(global|buffer|scratch|flat|tbuffer)_")
# non-VALU instructions whose first operand is a destination: they only tell the region-entry assumption that a register is
# not an input of the region (an instruction missing here only makes the check more cautious)
WRITES_FIRST = re.compile(r"^(s_(mov|cmov|add|addc|sub|subb|and|andn2|or|orn2|xor|nand|nor|xnor|not|cselect|lshl|lshr|ashr|mul|bfe|bfm|"
                          r"min|max|abs|load|buffer_load|getpc|brev|ff|flbit|bcnt|sext|movk)|ds_(read|bpermute|permute|swizzle)|"
                          r"(global|buffer|scratch|flat)_load)")
DPP_MOD = re.compile(r"\b(row_\w+|quad_perm|wave_\w+|row_bcast)\s*:")


def regs(tok):
    """registers named by one operand token, as strings: v[4:5] -> {v4, v5}; vcc -> {vcc_lo, vcc_hi}; s7 -> {s7}"""
    tok = tok.strip().lstrip("-!").strip("|")
    if tok.startswith(("neg(", "abs(", "sext(")):
        tok = tok[tok.index("(") + 1:].rstrip(")")
    m = re.match(r"^([vs])(\d+)$", tok)
    if m:
        return {tok}
    m = re.match(r"^([vs])\[(\d+):(\d+)\]$", tok)
    if m:
        return {"%s%d" % (m.group(1), i) for i in range(int(m.group(2)), int(m.group(3)) + 1)}
    if tok in ("vcc", "exec"):
        return {tok + "_lo", tok + "_hi"}
    if tok in ("vcc_lo", "vcc_hi", "exec_lo", "exec_hi", "m0"):
        return {tok}
    return set()


def is_sgpr(r):
    return r[0] == "s" or r.startswith(("vcc", "m0"))


class Insn:
    __slots__ = ("n", "text", "op", "defs", "uses", "ws", "region", "target", "falls", "kinds", "dpp", "writes")

    def __init__(self, n, text, region):
        self.n, self.text, self.region = n, text, region
        parts = text.split(None, 1)
        self.op = parts[0]
        ops = [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []
        ops = [o.split()[0] if o else o for o in ops]            # DPP / offset modifiers follow the last operand after a space
        self.ws = int(ops[0], 0) + 1 if self.op == "s_nop" and ops else 1
        self.target, self.falls = None, True
        m = re.search(r"(\.L[\w$.]+)\s*$", text)
        if self.op.startswith("s_cbranch") and m:
            self.target = m.group(1)
        elif self.op == "s_branch" and m:
            self.target, self.falls = m.group(1), False
        elif self.op in ("s_endpgm", "s_setpc_b64", "s_trap"):
            self.falls = False
        self.defs, self.uses = set(), []                          # uses: list of (register set, role)
        self.kinds = set()                                        # producer kinds of this instruction
        self.dpp = False
        self.writes = regs(ops[0]) if ops and WRITES_FIRST.match(self.op) else set()
        if not self.op.startswith("v_"):
            if VMEM.match(self.op):
                for o in ops:
                    rs = {r for r in regs(o) if is_sgpr(r)}
                    if rs:
                        self.uses.append((rs, "vmem"))
            return
        self.dpp = "_dpp" in self.op or bool(DPP_MOD.search(text))
        if self.op.startswith("v_permlane"):
            ndef = len(ops)
        elif TWO_DEFS.match(self.op):
            ndef = 2
        elif self.op.startswith(("v_nop", "v_interp")):
            ndef = 0
        else:
            ndef = 1 if ops else 0
        for o in ops[:ndef]:
            self.defs |= regs(o)
        if self.op.startswith("v_cmpx"):
            self.defs |= {"exec_lo", "exec_hi"}
        srcs = ops if self.op.startswith("v_permlane") else ops[ndef:]
        lanesel = self.op.startswith(("v_readlane", "v_writelane")) and len(ops) >= 3
        for i, o in enumerate(srcs):
            rs = regs(o)
            if not rs:
                continue
            if lanesel and i == len(srcs) - 1:
                self.uses.append((rs, "lanesel"))
            elif is_sgpr(next(iter(rs))):
                self.uses.append((rs, "sgpr"))
            else:
                self.uses.append((rs, "vgpr"))
        if self.op.startswith("v_div_fmas"):
            self.uses.append(({"vcc_lo", "vcc_hi"}, "div_fmas"))
        if any(is_sgpr(r) and not r.startswith("exec") for r in self.defs):
            self.kinds.add("sgpr")
        if any(r[0] == "v" and r[1:].isdigit() for r in self.defs):
            self.kinds.add("vgpr")
            if TRANS.match(self.op):
                self.kinds.add("trans")
        if any(r.startswith("exec") for r in self.defs):
            self.kinds.add("exec")

    def requirements(self):
        """[(rule, producer kind, wait states, registers)] that this instruction needs as a consumer"""
        out = []
        valu = self.op.startswith("v_")
        for rs, role in self.uses:
            if role == "vmem":
                out.append(("valu-sgpr>vmem", rs))
            elif role == "lanesel":
                out.append(("valu-sgpr>lanesel", rs))
            elif role == "div_fmas":
                out.append(("valu-vcc>div_fmas", rs))
            elif role == "sgpr":
                out.append(("valu-sgpr>valu", rs))
            elif role == "vgpr":
                out.append(("trans>valu", rs))
                if self.dpp:
                    out.append(("valu-vgpr>dpp", rs))
                if self.op.startswith(("v_readfirstlane", "v_readlane")):
                    out.append(("valu-vgpr>readlane", rs))
                if self.op.startswith("v_permlane"):
                    out.append(("valu-vgpr>permlane", rs))
        if valu and self.dpp:
            out.append(("valu-exec>dpp", {"exec_lo", "exec_hi"}))
        return [(rule, RULES[rule][0], RULES[rule][1], rs) for rule, rs in out]


def parse(path):
    """the instructions of one assembly file, with their predecessors"""
    insns, labels, kernel_first = [], {}, set()
    region, pending_labels, new_kernel = None, [], False
    with open(path) as f:
        for n, raw in enumerate(f, 1):
            s = raw.strip()
            if s.startswith(";;#ASMSTART"):
                region = n
                continue
            if s.startswith(";;#ASMEND"):
                region = None
                continue
            s = s.split(";")[0].strip()
            if not s:
                continue
            if KERNEL_START.match(raw) and not raw.startswith("."):
                new_kernel = True
            m = LABEL.match(s)
            if m:
                pending_labels.append(m.group(1))
                s = s[m.end():].strip()
                if not s:
                    continue
            if s.startswith("."):
                continue
            i = Insn(n, s, region)
            for lb in pending_labels:
                labels[lb] = len(insns)
            pending_labels = []
            if new_kernel:
                kernel_first.add(len(insns))
                new_kernel = False
            insns.append(i)
    preds = [[] for _ in insns]
    for k, i in enumerate(insns):
        if i.falls and k + 1 < len(insns) and k + 1 not in kernel_first:
            preds[k + 1].append(k)
        tgt = i.target
        if i.op == "s_setpc_b64":                                # branch relaxation: s_getpc; s_add (.LBB - .Lpost_getpc); s_setpc
            for j in range(max(0, k - 4), k):
                m = re.search(r"\((\.L\w+)-", insns[j].text)
                if m:
                    tgt = m.group(1)
        if tgt is not None and tgt in labels:
            preds[labels[tgt]].append(k)
    return insns, preds


def check_file(path, outside=False):
    """findings [(consumer line, producer line or None for the region-entry assumption, rule, distance, wait, text)]"""
    insns, preds = parse(path)
    found = {}
    for c, ci in enumerate(insns):
        if ci.op.startswith("v_") or ci.uses:
            reqs = ci.requirements()
        else:
            continue
        if not reqs:
            continue
        maxw = max(w for _, _, w, _ in reqs)
        # states: (node, distance so far, registers written inside the consumer's region on this path)
        stack = [(p, 0, frozenset()) for p in preds[c]]
        seen = set()
        while stack:
            p, d, written = stack.pop()
            if (p, d, written) in seen:
                continue
            seen.add((p, d, written))
            pi = insns[p]
            for rule, kind, w, rs in reqs:
                if d < w and kind in pi.kinds and rs & pi.defs:
                    if outside and (pi.region is not None or ci.region is not None):
                        continue
                    if not outside and pi.region is None and ci.region is None:
                        continue
                    key = (ci.n, rule)
                    if key not in found or found[key][3] > d:
                        found[key] = (ci.n, pi.n, rule, d, w, ci.text)
            d2 = d + pi.ws
            w2 = written | pi.defs | pi.writes if ci.region is not None and pi.region == ci.region else written
            if d2 >= maxw:
                continue
            for q in preds[p]:
                if ci.region is not None and pi.region == ci.region and insns[q].region != ci.region and not outside:
                    # leaving the consumer's region backwards: an unknown VALU instruction wrote every input of the region
                    for rule, kind, w, rs in reqs:
                        if d2 < w and kind != "exec" and not rs <= w2:
                            key = (ci.n, rule)
                            if key not in found or found[key][3] > d2:
                                found[key] = (ci.n, None, rule, d2, w, ci.text)
                stack.append((q, d2, w2))
        if ci.region is not None and not outside and (not preds[c] or any(insns[q].region != ci.region for q in preds[c])):
            # the consumer is the region's first instruction (or follows the compiler's code directly)
            for rule, kind, w, rs in reqs:
                if kind != "exec" and 0 < w:
                    key = (ci.n, rule)
                    found[key] = (ci.n, None, rule, 0, w, ci.text)
    return sorted(found.values())


def main():
    outside = "--outside" in sys.argv
    paths = [a for a in sys.argv[1:] if not a.startswith("--")] or sorted(glob.glob(os.path.join(OBJ, "*gfx950*.s")))
    if not paths:
        print("asm_hazards: no assembly found under %s (build with `make -C hmc.jl_amd/csrc`)" % OBJ)
        return 2
    bad = 0
    for p in paths:
        for cn, pn, rule, d, w, text in check_file(p, outside):
            bad += 1
            src = "region entry" if pn is None else "line %d" % pn
            print("%s:%d: [%s] %d of %d wait states after %s: %s" % (os.path.basename(p), cn, rule, d, w, src, text))
    print("asm_hazards: %d file(s), %d finding(s)%s" % (len(paths), bad, " in the compiler's own code" if outside else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
