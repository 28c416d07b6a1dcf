"""Predictive quantiles of the regime mixture (hmcg_predictive_quantiles[_device], include/hmcg_fan.h) without a GPU: the ABI
against the header, every misuse rule and their order from the built library, csrc/fan_plan.hpp run on the CPU (plain and under
sanitizers, as a stand-alone program) against the numpy cell choice and finish bit for bit, the numpy restatement against its
long-double CDF within the derived bounds of fan_cases, and the file route of hmc.calcfan with its writer."""
import ctypes as C
import datetime as dt
import os
import subprocess

import numpy as np
import pytest

import hmc_jl_amd
from hmc_jl_amd import _lib, hmc

import fan_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAN = _lib.Fan                        # the whole module is about this feature: without the binding none of it runs
ENTRIES = ["hmcg_predictive_quantiles", "hmcg_predictive_quantiles_device"]


def test_ctypes_struct_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    fields = ("nd", "nd_ld", "n_h", "n_p", "horizons", "rounds", "flags", "probs", "reserved")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%%zu", sizeof(hmcg_fan));\n%s\n'
                   'printf(" %%d %%d %%d %%d %%d %%d %%d %%d %%d", HMCG_FAN_ROUND5, HMCG_FAN_MAXP, HMCG_FAN_MAXROUNDS, HMCG_FAN_ROUNDS_DEFAULT, '
                   'HMCG_FAN_STRIDE, HMCG_FAN_NAN, HMCG_FAN_UNREACHED, HMCG_FAN_FLAT, HMCG_VERSION);return 0;}\n'
                   % (os.path.join(ROOT, "include", "hmcg_fan.h"),
                      "\n".join('printf(" %%zu", offsetof(hmcg_fan, %s));' % f for f in fields)))
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(FAN) == 216
    assert got[1:1 + len(fields)] == [getattr(FAN, f).offset for f in fields]
    assert got[1 + len(fields):-1] == [_lib.FAN_ROUND5, _lib.FAN_MAXP, _lib.FAN_MAXROUNDS, _lib.FAN_ROUNDS_DEFAULT, _lib.FAN_STRIDE,
                                       _lib.FAN_NAN, _lib.FAN_UNREACHED, _lib.FAN_FLAT] == [1, 16, 10, 4, 5, 1, 2, 4]
    lib = hmc_jl_amd.load()
    assert got[-1] == 109 == lib.hmcg_version()                # a companion header: the version stays
    assert _lib.FAN_EXPORTS == ("hmcg_predictive_quantiles", "hmcg_predictive_quantiles_device")
    assert not set(_lib.FAN_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.ORDER_EXPORTS) | set(_lib.ERGODIC_EXPORTS))
    for name in _lib.FAN_EXPORTS:
        assert getattr(lib, name).restype is C.c_int
    assert len(_lib.FAN_FIELDS) == _lib.FAN_STRIDE and (fc.NAN_, fc.UNREACHED, fc.FLAT) == (_lib.FAN_NAN, _lib.FAN_UNREACHED, _lib.FAN_FLAT)


def test_symbols_are_exported_by_the_built_library():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH]).decode()
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(_lib.FAN_EXPORTS) <= names


# In the header's order.  Fields overwritten on a good call (K = 3, nd = 40, horizons (0, 12), probs (0.1, 0.5)) | pointers
# withheld | text of the refusal.
MISUSE = [
    (dict(struct_size=7), {}, b"hmcg_fan.struct_size 7 != 216"),
    (dict(K=1), {}, b"K = 1 outside 2..8"),
    (dict(K=9), {}, b"K = 9 outside 2..8"),
    (dict(W=0), {}, b"W = 0: at least one window"),
    (dict(n_h=0), {}, b"n_h = 0 horizons outside 1..8"),
    (dict(n_h=9), {}, b"n_h = 9 horizons outside 1..8"),
    (dict(h1=-1), {}, b"horizon -1 outside 0..1024"),
    (dict(h1=1025), {}, b"horizon 1025 outside 0..1024"),
    (dict(n_p=0), {}, b"n_p = 0 probabilities outside 1..16"),
    (dict(n_p=17), {}, b"n_p = 17 probabilities outside 1..16"),
    (dict(p1=0.0), {}, b"probs[1] = 0 is not strictly inside (0, 1)"),
    (dict(p1=1.0), {}, b"probs[1] = 1 is not strictly inside (0, 1)"),
    (dict(p0=-0.25), {}, b"probs[0] = -0.25 is not strictly inside (0, 1)"),
    (dict(p1=float("nan")), {}, b"probs[1] = nan is not strictly inside (0, 1)"),
    (dict(p1=float("inf")), {}, b"probs[1] = inf is not strictly inside (0, 1)"),
    (dict(rounds=-1), {}, b"rounds = -1 outside 0..10"),
    (dict(rounds=11), {}, b"rounds = 11 outside 0..10"),
    (dict(nd=0, nd_ld=0), {}, b"nd = 0: at least one draw"),
    (dict(nd_ld=39), {}, b"nd_ld = 39 < nd = 40"),
    ({}, dict(mu=False), b"required"),
    ({}, dict(sig2=False), b"required"),
    ({}, dict(pi_end=False), b"required"),
    ({}, dict(out=False), b"required"),
    ({}, dict(range=False), b"required"),
    ({}, dict(flag=False), b"required"),
    ({}, dict(A=False), b"A is NULL with a horizon > 0"),
]
# Two rules broken at once: the rule the header names first.
DOUBLY_WRONG = [
    (dict(struct_size=7, K=1), {}, b"hmcg_fan.struct_size 7 != 216"),
    (dict(K=9, W=0), {}, b"K = 9 outside 2..8"),
    (dict(W=0, n_h=0), {}, b"W = 0: at least one window"),
    (dict(n_h=9, n_p=0), {}, b"n_h = 9 horizons outside 1..8"),
    (dict(h1=-1, n_p=17), {}, b"horizon -1 outside 0..1024"),
    (dict(n_p=17, p0=2.0), {}, b"n_p = 17 probabilities outside 1..16"),
    (dict(p0=2.0, rounds=11), {}, b"probs[0] = 2 is not strictly inside (0, 1)"),
    (dict(rounds=11, nd=0), {}, b"rounds = 11 outside 0..10"),
    (dict(nd=0, nd_ld=-1), {}, b"nd = 0: at least one draw"),
    (dict(nd_ld=39), dict(mu=False), b"nd_ld = 39 < nd = 40"),
    ({}, dict(flag=False, A=False), b"required"),
]


def _call(lib, entry, p, ptrs):
    buf = np.zeros(64)
    ok = C.c_void_p(buf.ctypes.data)
    a = [ok if ptrs.get(n, True) else None for n in ("mu", "sig2", "pi_end", "A", "out", "range", "flag")]
    return getattr(lib, entry)(p, *(a + ([None] if entry.endswith("device") else []) + [None]))


@pytest.mark.parametrize("entry", ENTRIES)
def test_misuse_is_refused_before_device_init(entry):
    """Every rule returns HMCG_E_BADARG with its text from the built library, a doubly wrong call the text of the rule the
    header names first; the data pointers are never followed (the device entry is handed host addresses here) and no GPU is
    needed: the check precedes get_context."""
    lib = hmc_jl_amd.load()
    for fields, ptrs, text in MISUSE + DOUBLY_WRONG:
        p = _lib.make_fan(1, 3, 40, 40, (0.1, 0.5), (0, 12))
        for k, v in fields.items():
            if k[0] == "h" and k[1:].isdigit():
                p.horizons[int(k[1:])] = v
            elif k[0] == "p" and k[1:].isdigit():
                p.probs[int(k[1:])] = v
            else:
                setattr(p, k, v)
        rc = _call(lib, entry, C.byref(p), ptrs)
        assert rc == -1 and text in lib.hmcg_last_error(), (fields, ptrs, rc, lib.hmcg_last_error())
    assert _call(lib, entry, None, {}) == -1 and b"hmcg_fan is NULL" in lib.hmcg_last_error()
    # A may be NULL when every horizon is 0: a call that is wrong elsewhere is then refused for that other reason
    p = _lib.make_fan(1, 3, 40, 40, (0.5,), (0, 0))
    rc = _call(lib, entry, C.byref(p), dict(A=False, mu=False))
    assert rc == -1 and b"required" in lib.hmcg_last_error()
    with pytest.raises(ValueError, match="at most 16 probabilities"):
        _lib.make_fan(1, 3, 40, 40, (0.5,) * 17)
    with pytest.raises(ValueError, match="at most 8 horizons"):
        _lib.make_fan(1, 3, 40, 40, (0.5,), (0,) * 9)
    with pytest.raises(ValueError, match="must share the shape"):
        _lib.predictive_quantiles(np.zeros((1, 3, 4)), np.zeros((1, 3, 5)), np.zeros((1, 3, 4)), None, (0.5,))


PLAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "%s"
using namespace hmcg_host;
static double rd() { unsigned long long u; if (std::scanf("%%llx", &u) != 1) std::exit(2); double x; memcpy(&x, &u, 8); return x; }
static void pr(double x, char end) { unsigned long long u; memcpy(&u, &x, 8); std::printf("%%016llx%%c", u, end); }
// stdin: lines "c first p lo hi Flo Fhi n F_0 .. F_{n-1}" (a cell choice and the finish on its result; doubles as 16 hex digits),
// "y lo hi M" (the M + 1 points of a bracket) and "r mu sig2" (the range terms).  stdout: one line per input line.
int main()
{
    hmcg_fan f{};
    f.rounds = 0;
    std::printf("%%d %%d %%d %%d %%d %%d %%zu\n", fan_rounds(f), fan_items_h(5, true), fan_items_h(5, false), fan_items(3, 5, true),
                fan_items(3, 5, false), fan_max_items(1, 2), fan_part_doubles(3, 2051, 2, 16));
    char kind;
    while (std::scanf(" %%c", &kind) == 1) {
        if (kind == 'c') {
            int first, n;
            if (std::scanf("%%d", &first) != 1) return 2;
            const double p = rd();
            double b[4] = {rd(), rd(), rd(), rd()};
            if (std::scanf("%%d", &n) != 1 || n != (first ? FAN_M1 + 1 : FAN_M - 1)) return 3;
            double F[FAN_M1 + 1];
            for (int i = 0; i < n; ++i) F[i] = rd();
            const int ms = fan_choose(b, F, first != 0, p);
            double q;
            const int fl = fan_finish(b, p, &q);
            std::printf("%%d %%d ", ms, fl);
            for (int i = 0; i < 4; ++i) pr(b[i], ' ');
            pr(q, '\n');
        } else if (kind == 'y') {
            const double lo = rd(), hi = rd();
            int M;
            if (std::scanf("%%d", &M) != 1) return 2;
            for (int m = 0; m <= M; ++m) pr(fan_point(lo, hi, M, m), m == M ? '\n' : ' ');
        } else if (kind == 'r') {
            const double mu = rd(), s2 = rd();
            double lo, hi;
            fan_reach(mu, s2, &lo, &hi);
            pr(lo, ' ');
            pr(hi, '\n');
        } else return 4;
    }
    return 0;
}
"""


def _hex(x):
    return "%016x" % int(np.float64(x).view(np.uint64))


def _unhex(h):
    return float(np.array([int(h, 16)], dtype=np.uint64).view(np.float64)[0])


def _same(a, b):
    return (np.isnan(a) and np.isnan(b)) or (a == b and np.signbit(a) == np.signbit(b))


def _tables():
    """Hand-made F tables: (name, first, p, (lo, hi, Flo, Fhi), F) -- a monotone ramp, a NaN at a point beside and on the chosen
    cell, a flat cell, an unreachable p, a tie F == p, a p below every value, a noisy non-monotone table."""
    out = []
    ramp1 = np.linspace(0.0, 1.0, 129) ** 2
    ramp = np.linspace(0.2, 0.3, 33)[1:32]
    b = (-3.0, 5.0, 0.2, 0.3)
    out.append(("ramp round 1", 1, 0.37, (-100.0, 150.0, 0.0, 0.0), ramp1))
    out.append(("ramp later", 0, 0.251, b, ramp))
    F = ramp1.copy(); F[40] = np.nan
    out.append(("NaN beside the cell", 1, 0.37, (-100.0, 150.0, 0.0, 0.0), F))
    m = int(np.flatnonzero(ramp1 >= 0.37)[0])
    F = ramp1.copy(); F[m] = np.nan                          # the NaN compares false: the next point is chosen, its lower end is the NaN
    out.append(("NaN on the cell", 1, 0.37, (-100.0, 150.0, 0.0, 0.0), F))
    F = ramp.copy(); F[9] = F[10] = 0.2505
    out.append(("flat cell", 0, 0.2505, b, F))              # two equal values: the first of them is chosen, its cell below it climbs
    F = ramp.copy(); F[:] = 0.2
    out.append(("flat everywhere below", 0, 0.25, (-3.0, 5.0, 0.2, 0.2), F))         # none >= p: the last cell, flat
    out.append(("unreachable", 0, 0.9, b, ramp))            # none >= p: the last cell; Fhi - Flo > 0, p > Fhi
    out.append(("unreachable round 1", 1, 0.999999, (0.0, 1.0, 0.0, 0.0), ramp1 * 0.99))
    out.append(("tie", 0, float(ramp[15]), b, ramp))        # F == p counts as reached
    out.append(("tie round 1", 1, float(ramp1[64]), (-100.0, 150.0, 0.0, 0.0), ramp1))
    out.append(("below every value", 0, 0.1, b, ramp))      # the first cell; p < Flo: the interpolation runs backwards, as written
    rng = np.random.default_rng(3)
    out.append(("noisy", 0, 0.25, b, ramp + rng.normal(0.0, 3e-3, 31)))
    out.append(("infinite bracket", 0, 0.25, (-np.inf, 5.0, 0.2, 0.3), ramp))
    out.append(("NaN end carried", 0, 0.9, (-3.0, 5.0, 0.2, np.nan), ramp))
    return out


def test_plan_header_on_the_cpu(tmp_path):
    """csrc/fan_plan.hpp, compiled by g++ -Wall -Werror into a stand-alone program and once more with
    -fsanitize=address,undefined (nothing is loaded into Python): fan_choose and fan_finish on the hand-made tables, fan_point
    and fan_reach print the bits of the numpy restatement -- the statements the kernels compile -- and the tables end as their
    names say."""
    src = tmp_path / "plan_main.cpp"
    src.write_text(PLAN_MAIN % os.path.join(ROOT, "hmc.jl_amd", "csrc", "fan_plan.hpp"))
    exe, san = tmp_path / "plan_main", tmp_path / "plan_main_san"
    flags = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror"]
    subprocess.check_call(flags + [str(src), "-o", str(exe)])
    subprocess.check_call(flags + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", str(src), "-o", str(san)])
    tables = _tables()
    brackets = [(-109.9091238, 112.4314438, 128), (-3.0, 5.0, 32), (1.0, 1.0 + 2.0 ** -50, 32), (2.5, 2.5, 128), (-np.inf, 1.0, 32), (-1e300, 1e300, 128)]
    reach = [(1.5, 0.04), (-2.25, 0.0), (np.nan, 1.0), (3.0, np.nan), (np.inf, 2.0), (0.1, 1e-5)]
    lines = ["c %d %s %s %d %s" % (first, _hex(p), " ".join(_hex(v) for v in b), len(F), " ".join(_hex(v) for v in F))
             for _, first, p, b, F in tables]
    lines += ["y %s %s %d" % (_hex(lo), _hex(hi), Mc) for lo, hi, Mc in brackets]
    lines += ["r %s %s" % (_hex(m), _hex(s)) for m, s in reach]
    text = ("\n".join(lines) + "\n").encode()
    out = subprocess.run([str(exe)], input=text, stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    assert subprocess.run([str(san)], input=text, stdout=subprocess.PIPE, check=True).stdout.decode().splitlines() == out
    # default rounds; items per (window, horizon) and per window in round 1 and later; the row of (n_h, n_p) = (1, 2); the work area
    assert [int(v) for v in out[0].split()] == [4, 129, 155, 387, 465, 129, 3 * 3 * 2 * 16 * 31]
    assert len(out) == 1 + len(lines)
    seen = {}
    for line, (name, first, p, b, F) in zip(out[1:], tables):
        tok = line.split()
        ms, fl, got = int(tok[0]), int(tok[1]), [_unhex(h) for h in tok[2:]]
        Mc = 128 if first else 32
        y = fc.points(b[0], b[1], Mc)
        Fall = np.asarray(F, dtype=np.float64) if first else np.concatenate(([b[2]], F, [b[3]]))
        cell = fc.choose(y, Fall, p)
        q, flag = fc.finish(*cell, p)
        assert fl == flag and all(_same(g, w) for g, w in zip(got, list(cell) + [q])), (name, ms, fl, got, cell, q, flag)
        assert _same(y[ms - 1], got[0]) and _same(y[ms], got[1])
        seen[name] = (ms, fl, got)
    assert seen["ramp round 1"][1] == 0 and seen["ramp later"][1] == 0 and seen["noisy"][1] == 0
    assert seen["NaN beside the cell"][1:] == seen["ramp round 1"][1:]
    assert seen["NaN on the cell"][1] == fc.NAN_ and np.isnan(seen["NaN on the cell"][2][4]) and seen["NaN on the cell"][0] == seen["ramp round 1"][0] + 1
    assert seen["flat cell"][:2] == (10, 0)
    assert seen["flat everywhere below"][:2] == (32, fc.FLAT) and seen["flat everywhere below"][2][4] == seen["flat everywhere below"][2][0]
    assert seen["unreachable"][:2] == (32, fc.UNREACHED) and seen["unreachable"][2][4] == 5.0
    assert seen["unreachable round 1"][:2] == (128, fc.UNREACHED) and seen["unreachable round 1"][2][4] == 1.0
    assert seen["tie"][:2] == (16, 0) and seen["tie"][2][4] == seen["tie"][2][1]               # q = hi exactly: (p - Flo) / (Fhi - Flo) = 1
    assert seen["tie round 1"][:2] == (64, 0)
    assert seen["below every value"][:2] == (1, 0) and seen["below every value"][2][4] < -3.0
    assert seen["NaN end carried"][:2] == (32, fc.NAN_)
    k = 1 + len(tables)
    for line, (lo, hi, Mc) in zip(out[k:], brackets):
        got = np.array([_unhex(h) for h in line.split()])
        want = fc.points(lo, hi, Mc)
        assert all(_same(g, w) for g, w in zip(got, want)), (lo, hi, Mc)
        assert _same(got[Mc], hi)
    k += len(brackets)
    for line, (m, s) in zip(out[k:], reach):
        got = [_unhex(h) for h in line.split()]
        with np.errstate(invalid="ignore"):
            r = 40.0 * np.sqrt(np.float64(s))
            assert _same(got[0], np.float64(m) - r) and _same(got[1], np.float64(m) + r)


@pytest.mark.parametrize("seed,K,nd,spread,horizons,probs,rounds", fc.CPU_CASES)
def test_reference_within_the_acceptance(seed, K, nd, spread, horizons, probs, rounds):
    """The float64 restatement on the case table meets what the GPU tests ask of the device -- |F_ld(q) - p| <= B + 4 tolF, the
    bracket width, lo <= q <= hi, the end values on their sides of p -- so the inputs keep the reference inside the acceptance."""
    mu, sig2, pi, A = fc.make_draws(seed, 1, K, nd, 0, max(horizons) > 0, spread)
    out, rng, flag = fc.reference(mu, sig2, pi, A, probs, horizons, rounds, True)
    assert (flag == 0).all() and np.isfinite(out).all() and np.isfinite(rng).all()
    worst = fc.check_block(out, rng, flag, probs, horizons, rounds, nd, K, fc.judge(mu, sig2, pi, A, horizons, True), "cpu")
    print("K=%d nd=%d spread=%g h=%s R=%d: max |F_ld(q) - p| / (B + 4 tolF) = %.3g" % (K, nd, spread, horizons, rounds, worst))
    q = out[..., 0]
    order = np.argsort(np.asarray(probs), kind="stable")
    assert (np.diff(q[..., order], axis=-1) >= 0.0).all()      # quantiles ascend with p
    if 0 in horizons and horizons.count(0) > 1:
        js = [j for j, h in enumerate(horizons) if h == 0]
        assert np.array_equal(out[:, js[0]], out[:, js[1]])


def test_reference_edge_inputs():
    """What the GPU edge test expects of the device, from the restatement alone: a NaN mean under a zero weight poisons every F
    (flag NAN, q NaN) while the range ignores it; weights rounded to sum below p: no F reaches p -- with regimes far enough
    apart that round 1's last cell still climbs the flag is UNREACHED and q = hi0, otherwise Phi has saturated at exactly 1
    below hi0 and the last cell is FLAT; a zero rounded variance is a jump the bracket closes on."""
    K, nd = 2, 70
    mu, sig2, pi, _ = fc.make_draws(5, 1, K, nd, 0, False)
    mu[0, 1, 9], pi[0, 0, 9], pi[0, 1, 9] = np.nan, 1.0, 0.0
    out, rng, flag = fc.reference(mu, sig2, pi, None, (0.5,), (0,), 2, True)
    assert (flag == fc.NAN_).all() and np.isnan(out[..., 0]).all() and np.isfinite(rng).all()
    mu2, sig22 = np.zeros((1, 2, 33)), np.ones((1, 2, 33))
    mu2[0, 1] = 10000.0
    pi2 = np.full((1, 2, 33), 0.499994)                          # rounds to 0.49999: the weights sum to 0.99998 < 1 - 1e-6
    out, rng, flag = fc.reference(mu2, sig22, pi2, None, (1 - 1e-6,), (0,), 1, True)
    assert flag[0, 0, 0] == fc.UNREACHED and out[0, 0, 0, 0] == rng[0, 1] == 10040.0 and abs(out[0, 0, 0, 4] - 0.99998) < 1e-14
    out, rng, flag = fc.reference(mu2, sig22, pi2, None, (1 - 1e-6, 0.5), (0,), 4, True)
    assert flag[0, 0, 0] == fc.FLAT and flag[0, 0, 1] == 0 and out[0, 0, 0, 0] == out[0, 0, 0, 1] < rng[0, 1]
    mu3, sig23, pi3, _ = fc.make_draws(6, 1, 2, 40, 0, False)
    mu3[0, :, :], sig23[0, 0, :], sig23[0, 1, :] = np.array([[1.37], [4.0]]), 4e-6, 1.0
    pi3[0, 0, :], pi3[0, 1, :] = 0.6, 0.4                        # a jump of 0.6 at 1.37, which no point hits (on it F is NaN, as in the CDF entry)
    out, rng, flag = fc.reference(mu3, sig23, pi3, None, (0.3,), (0,), 6, True)
    assert flag[0, 0, 0] == 0 and out[0, 0, 0, 1] <= 1.37 <= out[0, 0, 0, 2] and abs(out[0, 0, 0, 0] - 1.37) <= out[0, 0, 0, 2] - out[0, 0, 0, 1]


def _hand_made(seed, K=3, n=300):
    """Draws in the reference's Julia shapes: means, variances, states (n, K), A (n, K, K) with A[d, i, j]."""
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((n, K)) + 3.0 * np.arange(K)
    variances = 0.05 + rng.gamma(2.0, 0.8, size=(n, K))
    states = rng.dirichlet(np.ones(K), size=n)
    A = 0.1 * rng.dirichlet(np.ones(K) * 2.0, size=(n, K)) + 0.9 * np.eye(K)
    return means, variances, states, A


def test_calcfan_file_route_and_writer(tmp_path):
    """Per-draw files written by hmc.saveresults from hand-made draws (K = 3, n = 300, two dates) through hmc.calcfan (numpy,
    no GPU): its blocks are fan_cases.reference's on the same draws rounded as the cells are, bit for bit -- two restatements
    of the header written apart --, they pass the acceptance the device is held to, and the bands nest; then the writer's text."""
    dates = [dt.date(1980, 1, 1), dt.date(1985, 1, 1)]
    draws = [_hand_made(71 + i) for i in range(2)]
    for d, (means, variances, states, A) in zip(dates, draws):
        n, K = means.shape
        ds = [dt.date(1960 + i // 12, i % 12 + 1, 1) for i in range(11)] + [d]
        opt = hmc.estopt(np.zeros(12), ds, sampleRange=range(1, 13), endIndex=12, horizons=(12,), D=K, burnin=1, Nrun=n)
        hmc.saveresults(hmc.Samples(means, variances, states[:, None, :], A, np.zeros((n, 2)), [d] * n), opt, str(tmp_path), native=False)
    mu, sig2 = np.stack([m.T for m, _, _, _ in draws]), np.stack([v.T for _, v, _, _ in draws])
    pi = np.stack([s.T for _, _, s, _ in draws])
    A = np.stack([np.transpose(a, (2, 1, 0)) for _, _, _, a in draws])
    horizons = (0, 12)
    got_dates, f = hmc.calcfan(str(tmp_path), dates, fc.PROBS5, horizons)
    assert got_dates == [str(x) for x in dates] and f["quantile"].shape == (2, 2, 5) and f["rounds"] == 0
    out, rng, flag = fc.reference(mu, sig2, pi, A, fc.PROBS5, horizons, 0, True)
    for i, name in enumerate(_lib.FAN_FIELDS):
        assert np.array_equal(f[name], out[..., i]), name
    assert np.array_equal(f["range"], rng) and np.array_equal(f["flag"], flag) and (flag == 0).all()
    fc.check_block(out, rng, flag, fc.PROBS5, horizons, 0, 300, 3, fc.judge(mu, sig2, pi, A, horizons, True), "files")
    q = f["quantile"]
    assert (np.diff(q, axis=2) > 0.0).all()                    # 2.5 % < 16 % < median < 84 % < 97.5 %
    two = hmc.calcfan(str(tmp_path), dates[1:], (0.5,), (12,), rounds=2)[1]
    assert abs(two["quantile"][0, 0, 0] - q[1, 1, 2]) <= two["hi"][0, 0, 0] - two["lo"][0, 0, 0]
    with pytest.raises(FileNotFoundError):
        hmc.calcfan(str(tmp_path), [dt.date(1990, 1, 1)], (0.5,))
    with pytest.raises(ValueError, match="strictly inside"):
        hmc.calcfan(str(tmp_path), dates, (0.5, 1.0))
    with pytest.raises(ValueError, match="rounds outside"):
        hmc.calcfan(str(tmp_path), dates, (0.5,), rounds=11)
    path = hmc.write_fan(str(tmp_path / "fan.csv"), got_dates, f)
    header, rows = hmc._read_csv(path)
    assert header == ["date", "horizon", "p", "quantile", "lo", "hi", "flag"] and len(rows) == 2 * 2 * 5
    r = rows[5 * 2 + 5 + 2]
    assert r == ["1985-01-01", "12", "0.5", hmc._fmt(q[1, 1, 2]), hmc._fmt(f["lo"][1, 1, 2]), hmc._fmt(f["hi"][1, 1, 2]), "0"]


def test_batchresult_fan_is_none_unless_asked_for():
    res = hmc.BatchResult([], {"summary": np.zeros((0, 1)), "status": np.zeros(0, dtype=np.int32)}, False)
    assert res.fan is None
    with pytest.raises(ValueError, match="no predictive quantiles"):
        hmc.calcfan("unused", ["1980-01-01"], (0.5,), result=res)
