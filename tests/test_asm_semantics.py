"""What the generated K = 8 assembly computes in the blocks that were reordered to pad their VCC hazards, checked on the CPU
by executing the instructions of the shipped .inc files (a small lane-parallel interpreter for the handful of opcodes these
blocks use) against the C++ definition of the same operation.

Why on the CPU: two of the three blocks cannot be reached through the library's API, so no GPU test can make them take
their other branch.
  * The product's rescale clamp (e = 1022 - be when 0 < be < 2040, else 0).  The pdf pass scales every step's pdfs so that
    the largest lies in [0.5, 1) (or sets them all to 1), and every row of A diag(f) then sums to at most 1, so the 8-step
    product's largest entry is below 2 (be <= 1023).  It is at least (0.5 min A)^8 / 8, so be = 0 needs an entry of A below
    ~1e-38, and A's rows are Dirichlet(counts + 1) draws.
  * The replay's rare path (total = sum_s c[s] f[s] not > 0).  With sum_r pif[t-1, r] = 1, c[s*] >= min_r A[r][s*] for the
    state s* whose f >= 0.5, so total >= min A / 2: an entry of A below ~1e-323 would be needed.
The third block, the eps() guard, is reached at most steps by tests/test_gpu_k8_edges.py; here it is checked at the edges
(eps itself, its neighbours, 0, subnormals, NaN) as well."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hmc.jl_amd", "csrc")
EPS = float(np.finfo(np.float64).eps)


def inc_lines(name):
    return [ln.strip()[1:].split("\\n")[0] for ln in open(os.path.join(CSRC, name)) if ln.strip().startswith('"')]


class Lanes:
    """per-lane 32-bit registers (VGPRs, SGPRs, operand placeholders %[x]); SGPR pairs used as lane masks hold booleans"""

    def __init__(self, n):
        self.n, self.r = n, {}
        self.exec = np.ones(n, dtype=bool)

    @property
    def all_on(self):
        return bool(self.exec.all())

    def u32(self, tok):
        if re.match(r"^-?(0x[0-9a-f]+|\d+)$", tok):
            return np.uint32(int(tok, 0) & 0xFFFFFFFF)
        return self.r[tok.replace("%[", "%").rstrip("]")]

    def f64(self, tok):
        m = re.match(r"^([vs])\[(\d+):(\d+)\]$", tok)
        lo, hi = self.r["%s%d" % (m.group(1), int(m.group(2)))], self.r["%s%d" % (m.group(1), int(m.group(3)))]
        return ((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)).view(np.float64)

    def mask(self, tok):
        return self.r[re.sub(r"^s\[(\d+):\d+\]$", r"s\1", tok)]

    def set_f64(self, tok, x):
        m = re.match(r"^([vs])\[(\d+):(\d+)\]$", tok)
        b = np.asarray(x, dtype=np.float64).view(np.uint64)
        self.r["%s%s" % (m.group(1), m.group(2))] = (b & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        self.r["%s%s" % (m.group(1), m.group(3))] = (b >> np.uint64(32)).astype(np.uint32)

    def write(self, tok, val):
        key = tok.replace("%[", "%").rstrip("]")
        val = np.asarray(val, dtype=np.uint32)
        if self.all_on:
            self.r[key] = val if val.shape == (self.n,) else np.full(self.n, val, dtype=np.uint32)
        else:
            self.r[key] = np.where(self.exec, val, self.r.get(key, np.zeros(self.n, dtype=np.uint32)))

    def write_mask(self, tok, val):
        self.r[re.sub(r"^s\[(\d+):\d+\]$", r"s\1", tok)] = val if self.all_on else val & self.exec   # 0 for inactive lanes

    def run(self, lines):
        for ln in lines:
            op, rest = (ln.split(None, 1) + [""])[:2]
            a = [t.strip() for t in rest.split(",")] if rest else []
            if op == "v_add_u32":
                self.write(a[0], self.u32(a[1]) + self.u32(a[2]))
            elif op == "v_sub_u32":
                self.write(a[0], self.u32(a[1]) - self.u32(a[2]))
            elif op == "v_lshrrev_b32":
                self.write(a[0], self.u32(a[2]) >> self.u32(a[1]))
            elif op == "v_or_b32":
                self.write(a[0], self.u32(a[1]) | self.u32(a[2]))
            elif op == "v_mov_b32":
                self.write(a[0], self.u32(a[1]))
            elif op == "v_bfi_b32":
                m = self.u32(a[1])
                self.write(a[0], (m & self.u32(a[2])) | (~m & self.u32(a[3])))
            elif op == "v_cndmask_b32":
                self.write(a[0], np.where(self.mask(a[3]), self.u32(a[2]), self.u32(a[1])))
            elif op == "v_cmp_gt_u32":
                self.write_mask(a[0], self.u32(a[1]) > self.u32(a[2]))
            elif op == "v_cmp_gt_i32":
                self.write_mask(a[0], self.u32(a[1]).view(np.int32) > self.u32(a[2]).view(np.int32))
            elif op == "v_cmp_lt_f64":
                self.write_mask(a[0], self.f64(a[1]) < self.f64(a[2]))
            elif op == "s_and_saveexec_b64":
                self.r[re.sub(r"^s\[(\d+):\d+\]$", r"s\1", a[0])] = self.exec.copy()
                self.exec = self.exec & self.mask(a[1])
            elif op == "s_mov_b64" and a[0] == "exec":
                self.exec = self.mask(a[1]).copy()
            else:
                raise AssertionError("opcode outside the interpreter: " + ln)


def block(lines, first, last):
    """lines[i..j] from the first line matching `first` to the next one matching `last` (inclusive)"""
    i = next(k for k, ln in enumerate(lines) if re.search(first, ln))
    j = next(k for k in range(i, len(lines)) if re.search(last, lines[k]))
    return lines[i:j + 1]


def test_product_rescale_clamp_over_every_high_word():
    """The exponent the rescale of product_asm_k8.inc applies, for every 32-bit high word of the row's largest entry,
    equals rescale_pow2's (gibbs_device.hpp): 1022 - be when 0 < be < 2040, else 0 -- be = 0, 2040..2047 and the sign
    bit (be >= 2048) included."""
    lines = inc_lines("product_asm_k8.inc")
    clamp = block(lines, r"^v_max_u32 v241, v241, v127$", r"^v_cndmask_b32 v242")[1:]
    assert [ln.split()[0] for ln in clamp] == ["v_add_u32", "v_cmp_gt_u32", "v_lshrrev_b32", "v_sub_u32", "v_cndmask_b32"]
    n = 1 << 24
    base = np.arange(n, dtype=np.uint32)
    for c in range(1 << 8):
        hi = base + np.uint32(c * n)
        L = Lanes(n)
        L.r["v241"] = hi
        L.run(clamp)
        be = (hi >> np.uint32(20)).astype(np.int32)
        want = np.where((be > 0) & (be < 2040), 1022 - be, 0).astype(np.int32)
        assert np.array_equal(L.r["v242"].view(np.int32), want), c


def eps_guard_case(av, idx, u):
    """runs the first eps() guard of replay_asm_k8.inc on lanes with pif[t, :] = av (n, 8), the categorical draws idx
    (n, 8) and the uniform-law draw u (n,); returns the merged map word"""
    lines = inc_lines("replay_asm_k8.inc")
    guard = block(lines, r"^v_cmp_lt_f64 s\[20:21\], s\[18:19\], v\[0:1\]$", r"^v_bfi_b32 v216")
    n = av.shape[0]
    L = Lanes(n)
    L.set_f64("s[18:19]", np.full(n, EPS))
    for s in range(8):
        L.set_f64("v[%d:%d]" % (2 * s, 2 * s + 1), av[:, s])
        L.r["v%d" % (226 + s)] = np.full(n, (0xF << (4 * s)) & 0xFFFFFFFF, dtype=np.uint32)
    L.r["v220"] = np.zeros(n, dtype=np.uint32)
    L.r["v218"] = (u.astype(np.uint32) * np.uint32(0x11111111))                       # floor(8 u) in every nibble
    L.r["v216"] = sum((idx[:, s].astype(np.uint32) << np.uint32(4 * s)) for s in range(8)).astype(np.uint32)
    L.run(guard)
    return L.r["v216"]


def test_replay_eps_guard_at_the_edges():
    """nibble s of the map is the categorical draw when pif[t, s] > eps(), the uniform draw otherwise (:472-480) -- with
    every label's value drawn from eps() itself, its neighbours, 0, -0, the smallest subnormal, NaN and ordinary values,
    so that neighbouring labels straddle eps() in every combination"""
    rng = np.random.default_rng(3)
    edge = np.array([EPS, np.nextafter(EPS, 0), np.nextafter(EPS, 1), 0.0, -0.0, 5e-324, EPS / 2, 2 * EPS, 1e-300,
                     1e-10, 0.5, 1.0, np.nan])
    n = 200000
    av = edge[rng.integers(0, len(edge), size=(n, 8))]
    idx = rng.integers(0, 8, size=(n, 8))
    u = rng.integers(0, 8, size=n)
    got = eps_guard_case(av, idx, u)
    want = np.zeros(n, dtype=np.uint32)
    for s in range(8):
        nib = np.where(av[:, s] > EPS, idx[:, s], u).astype(np.uint32)
        want |= nib << np.uint32(4 * s)
    assert np.array_equal(got, want)
    straddle = ((av[:, 1:] > EPS) != (av[:, :-1] > EPS)).any(axis=1)
    assert straddle.mean() > 0.9


@pytest.mark.parametrize("tag", ["p", "1", "0"])
def test_replay_rare_path(tag):
    """the three rare blocks of replay_asm_k8.inc: on the lanes whose total is not > 0 (vcc), the uniform law (every nv = 1/8,
    total = 1) and the emission-underflow flag when the lane's step t = l + t0 is < T; the other lanes and exec unchanged"""
    lines = inc_lines("replay_asm_k8.inc")
    rare = block(lines, r"^\.Lhmcg_rep_rare%s_%%=:$" % tag, r"^s_mov_b64 exec, s\[20:21\]$")[1:]
    rng = np.random.default_rng(5)
    n, T, flag = 4096, 3001, 2
    L = Lanes(n)
    vcc = rng.random(n) < 0.5
    L.r["vcc"] = vcc.copy()
    l = np.full(n, 7, dtype=np.uint32)
    t0 = rng.integers(T - 200, T + 200, size=n).astype(np.uint32)
    st = rng.integers(0, 64, size=n).astype(np.uint32) & ~np.uint32(flag)
    L.r.update({"%l": l, "%t0": t0, "%T": np.full(n, T, dtype=np.uint32), "%flagv": np.full(n, flag, dtype=np.uint32),
                "%st": st.copy()})
    before = {}
    for r in list(range(80, 96)) + [208, 209, 225]:
        L.r["v%d" % r] = before[r] = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    L.run(rare)
    assert L.exec.all()
    for s in range(8):
        nv = L.f64("v[%d:%d]" % (80 + 2 * s, 81 + 2 * s))
        assert (nv[vcc] == 0.125).all()
        assert np.array_equal(L.r["v%d" % (80 + 2 * s)][~vcc], before[80 + 2 * s][~vcc])
        assert np.array_equal(L.r["v%d" % (81 + 2 * s)][~vcc], before[81 + 2 * s][~vcc])
    tot = L.f64("v[208:209]")
    assert (tot[vcc] == 1.0).all() and np.array_equal(L.r["v208"][~vcc], before[208][~vcc])
    flagged = vcc & ((l + t0).astype(np.int64) < T)
    assert np.array_equal(L.r["%st"], np.where(flagged, st | flag, st))
    assert flagged.any() and (vcc & ~flagged).any()
