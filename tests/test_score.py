"""Proper scores of the predictive regime mixture (hmcg_predictive_scores[_device], include/hmcg_score.h) without a GPU: the ABI
against the header, every misuse rule and their order from the built library, csrc/score_plan.hpp run on the CPU (plain and
under sanitizers, as a stand-alone program) against Python restatements, the reference of score_cases against closed forms and
a long-double quadrature, and the file route of hmc.calcscores with its writer and summary."""
import ctypes as C
import datetime as dt
import math
import os
import subprocess

import numpy as np
import pytest

import hmc_jl_amd
from hmc_jl_amd import _lib, hmc

import fan_cases as fc
import predictive_cases as pc
import score_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE = _lib.Score                    # the whole module is about this feature: without the binding none of it runs
ENTRIES = ["hmcg_predictive_scores", "hmcg_predictive_scores_device"]
LD = np.longdouble


def test_ctypes_struct_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    fields = ("struct_size", "W", "K", "device", "nd", "nd_ld", "n_h", "flags", "horizons", "stride", "reserved")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%%zu", sizeof(hmcg_score));\n%s\n'
                   'printf(" %%d %%d %%d %%d", HMCG_SCORE_ROUND5, HMCG_SCORE_DRAWS_DEFAULT, HMCG_SCORE_STRIDE, HMCG_VERSION);return 0;}\n'
                   % (os.path.join(ROOT, "include", "hmcg_score.h"),
                      "\n".join('printf(" %%zu", offsetof(hmcg_score, %s));' % f for f in fields)))
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(SCORE) == 88
    assert got[1:1 + len(fields)] == [getattr(SCORE, f).offset for f in fields]
    assert got[1 + len(fields):-1] == [_lib.SCORE_ROUND5, _lib.SCORE_DRAWS_DEFAULT, _lib.SCORE_STRIDE] == [1, 4096, 5]
    assert SCORE.stride.size == 8
    lib = hmc_jl_amd.load()
    assert got[-1] == 109 == lib.hmcg_version()                # a companion header: the version stays
    assert _lib.SCORE_EXPORTS == ("hmcg_predictive_scores", "hmcg_predictive_scores_device")
    assert not set(_lib.SCORE_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.ORDER_EXPORTS) | set(_lib.ERGODIC_EXPORTS) | set(_lib.FAN_EXPORTS))
    for name in _lib.SCORE_EXPORTS:
        assert getattr(lib, name).restype is C.c_int
    assert _lib.SCORE_FIELDS == sc.FIELDS == ("crps", "e_abs", "e_pair", "pit", "pdf") and len(_lib.SCORE_FIELDS) == _lib.SCORE_STRIDE


def test_symbols_are_exported_by_the_built_library():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH]).decode()
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(_lib.SCORE_EXPORTS) <= names


# In the header's order.  Fields overwritten on a good call (K = 3, nd = 40, horizons (0, 12)) | pointers withheld | text of the
# refusal.
MISUSE = [
    (dict(struct_size=7), {}, b"hmcg_score.struct_size 7 != 88"),
    (dict(K=1), {}, b"K = 1 outside 2..8"),
    (dict(K=9), {}, b"K = 9 outside 2..8"),
    (dict(W=0), {}, b"W = 0: at least one window"),
    (dict(n_h=0), {}, b"n_h = 0 horizons outside 1..8"),
    (dict(n_h=9), {}, b"n_h = 9 horizons outside 1..8"),
    (dict(h1=-1), {}, b"horizon -1 outside 0..1024"),
    (dict(h1=1025), {}, b"horizon 1025 outside 0..1024"),
    (dict(nd=0, nd_ld=0), {}, b"nd = 0: at least one draw"),
    (dict(nd_ld=39), {}, b"nd_ld = 39 < nd = 40"),
    (dict(stride=-1), {}, b"stride = -1 is negative"),
    (dict(W=1000, K=8, nd=10 ** 9, nd_ld=10 ** 9, stride=1), {}, b"exceeds one launch (2^31 - 1 blocks)"),
    (dict(W=2 ** 31 - 1, nd=2 * 4096 * 1024 + 1, nd_ld=2 * 4096 * 1024 + 1), {}, b"exceeds one launch (2^31 - 1 blocks)"),
    ({}, dict(mu=False), b"required"),
    ({}, dict(sig2=False), b"required"),
    ({}, dict(pi_end=False), b"required"),
    ({}, dict(yreal=False), b"required"),
    ({}, dict(out=False), b"required"),
    ({}, dict(A=False), b"A is NULL with a horizon > 0"),
]
# Two rules broken at once: the rule the header names first.
DOUBLY_WRONG = [
    (dict(struct_size=7, K=1), {}, b"hmcg_score.struct_size 7 != 88"),
    (dict(K=9, W=0), {}, b"K = 9 outside 2..8"),
    (dict(W=0, n_h=0), {}, b"W = 0: at least one window"),
    (dict(n_h=9, nd=0), {}, b"n_h = 9 horizons outside 1..8"),
    (dict(h1=-1, stride=-1), {}, b"horizon -1 outside 0..1024"),
    (dict(nd=0, nd_ld=-1), {}, b"nd = 0: at least one draw"),
    (dict(nd_ld=39, stride=-2), {}, b"nd_ld = 39 < nd = 40"),
    (dict(stride=-2), dict(mu=False), b"stride = -2 is negative"),
    (dict(W=1000, K=8, nd=10 ** 9, nd_ld=10 ** 9, stride=1), dict(out=False), b"exceeds one launch"),
    ({}, dict(yreal=False, A=False), b"required"),
]


def _call(lib, entry, p, ptrs):
    buf = np.zeros(64)
    ok = C.c_void_p(buf.ctypes.data)
    a = [ok if ptrs.get(n, True) else None for n in ("mu", "sig2", "pi_end", "A", "yreal", "out")]
    return getattr(lib, entry)(p, *(a + ([None] if entry.endswith("device") else []) + [None]))


@pytest.mark.parametrize("entry", ENTRIES)
def test_misuse_is_refused_before_device_init(entry):
    """Every rule returns HMCG_E_BADARG with its text from the built library, a doubly wrong call the text of the rule the
    header names first; the data pointers are never followed (the device entry is handed host addresses here) and no GPU is
    needed: the check precedes get_context."""
    lib = hmc_jl_amd.load()
    for fields, ptrs, text in MISUSE + DOUBLY_WRONG:
        p = _lib.make_score(1, 3, 40, 40, (0, 12))
        for k, v in fields.items():
            if k[0] == "h" and k[1:].isdigit():
                p.horizons[int(k[1:])] = v
            else:
                setattr(p, k, v)
        rc = _call(lib, entry, C.byref(p), ptrs)
        assert rc == -1 and text in lib.hmcg_last_error(), (fields, ptrs, rc, lib.hmcg_last_error())
    assert _call(lib, entry, None, {}) == -1 and b"hmcg_score is NULL" in lib.hmcg_last_error()
    # A may be NULL when every horizon is 0: a call that is wrong elsewhere is then refused for that other reason
    p = _lib.make_score(1, 3, 40, 40, (0, 0))
    rc = _call(lib, entry, C.byref(p), dict(A=False, mu=False))
    assert rc == -1 and b"required" in lib.hmcg_last_error()
    with pytest.raises(ValueError, match="at most 8 horizons"):
        _lib.make_score(1, 3, 40, 40, (0,) * 9)
    with pytest.raises(ValueError, match="must share the shape"):
        _lib.predictive_scores(np.zeros((1, 3, 4)), np.zeros((1, 3, 5)), np.zeros((1, 3, 4)), None, None)
    with pytest.raises(ValueError, match="yreal must have the shape"):
        _lib.predictive_scores(np.ones((1, 3, 4)), np.ones((1, 3, 4)), np.ones((1, 3, 4)), None, np.zeros((2, 1)))


PLAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "%s"
using namespace hmcg_host;
static double rd() { unsigned long long u; if (std::scanf("%%llx", &u) != 1) std::exit(2); double x; memcpy(&x, &u, 8); return x; }
static void pr(double x, char end) { unsigned long long u; memcpy(&u, &x, 8); std::printf("%%016llx%%c", u, end); }
// stdin: lines "t nd stride" (the thinning), "p nT" (the row pairing: per block its rows), "w n_u K n_h" (the work area),
// "g W n_u ncol cap" (windows per group) and "a m S2" (doubles as 16 hex digits).  stdout: one line per input line.
int main()
{
    char kind;
    while (std::scanf(" %%c", &kind) == 1) {
        if (kind == 't') {
            long long nd, st;
            if (std::scanf("%%lld %%lld", &nd, &st) != 2) return 2;
            std::printf("%%lld %%lld\n", score_stride(nd, st), score_used(nd, st));
        } else if (kind == 'p') {
            long long nT;
            if (std::scanf("%%lld", &nT) != 1) return 2;
            const long long N = nT * SCORE_TP - 3;
            if (score_tiles(N) != nT) return 5;
            std::vector<int> seen((size_t)nT, 0);
            for (long long b = 0; b < score_blocks(N); ++b) {
                long long r[2];
                const int n = score_rows(nT, b, r);
                for (int i = 0; i < n; ++i) { std::printf("%%lld%%c", r[i], i + 1 == n ? ';' : ','); seen[(size_t)r[i]]++; }
            }
            for (long long r = 0; r < nT; ++r) if (seen[(size_t)r] != 1) return 6;
            std::printf("\n");
        } else if (kind == 'w') {
            long long n_u; int K, n_h;
            if (std::scanf("%%lld %%d %%d", &n_u, &K, &n_h) != 3) return 2;
            const ScoreWork s = score_work(n_u, K, n_h);
            std::printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu\n", s.o_mu, s.o_v, s.o_w, s.o_lin, s.o_pair, s.total, score_work_doubles(3, n_u, K, n_h));
        } else if (kind == 'g') {
            int W, ncol; long long n_u, cap;
            if (std::scanf("%%d %%lld %%d %%lld", &W, &n_u, &ncol, &cap) != 4) return 2;
            std::printf("%%d\n", score_group_windows(W, n_u, ncol, cap));
        } else if (kind == 'a') {
            const double m = rd(), S2 = rd();
            pr(score_a(m, S2), '\n');
        } else return 4;
    }
    return 0;
}
"""


def _hex(x):
    return "%016x" % int(np.float64(x).view(np.uint64))


def _unhex(h):
    return float(np.array([int(h, 16)], dtype=np.uint64).view(np.float64)[0])


THINNING = [(1, 0, 1, 1), (4096, 0, 1, 4096), (4097, 0, 2, 2049), (8209, 0, 3, 2737), (250000, 0, 62, 4033),
            (250000, 1, 1, 250000), (10, 3, 3, 4), (9, 3, 3, 3), (5, 7, 7, 1)]


def test_plan_header_on_the_cpu(tmp_path):
    """csrc/score_plan.hpp, compiled by g++ -Wall -Werror into a stand-alone program and once more with
    -fsanitize=address,undefined (nothing is loaded into Python): the thinning, the row pairing (every row of tiles in exactly
    one block, so every tile pair on or below the diagonal is visited once), the work area, the window groups and a(m, S2)
    against their Python restatements."""
    src = tmp_path / "plan_main.cpp"
    src.write_text(PLAN_MAIN % os.path.join(ROOT, "hmc.jl_amd", "csrc", "score_plan.hpp"))
    exe, san = tmp_path / "plan_main", tmp_path / "plan_main_san"
    flags = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror"]
    subprocess.check_call(flags + [str(src), "-o", str(exe)])
    subprocess.check_call(flags + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", str(src), "-o", str(san)])
    pairings = [1, 2, 3, 4, 7, 48, 129]
    works = [(1, 2, 1), (86, 3, 3), (1025, 8, 8), (4033, 3, 2), (2737, 2, 1)]
    groups = [(460, 4033, 18, 0), (460, 4033, 88, 0), (3, 50, 18, 0), (3, 50, 18, 1), (3, 50, 18, 2), (5, 10 ** 7, 88, 0), (7, 100, 9, 100)]
    rng = np.random.default_rng(9)
    avals = [(0.0, 0.0), (-2.5, 0.0), (0.0, 4.0), (1.0, 1.0), (-30.0, 0.5), (1e-9, 2.0), (np.nan, 1.0), (1.0, np.nan), (3.0, -1.0), (np.inf, 1.0),
             (1e3, 1e-10)] + [(float(rng.normal(0, 3)), float(rng.gamma(2.0, 1.0))) for _ in range(200)]
    lines = ["t %d %d" % (nd, st) for nd, st, _, _ in THINNING] + ["p %d" % n for n in pairings]
    lines += ["w %d %d %d" % w for w in works] + ["g %d %d %d %d" % g for g in groups] + ["a %s %s" % (_hex(m), _hex(s)) for m, s in avals]
    text = ("\n".join(lines) + "\n").encode()
    out = subprocess.run([str(exe)], input=text, stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    assert subprocess.run([str(san)], input=text, stdout=subprocess.PIPE, check=True).stdout.decode().splitlines() == out
    assert len(out) == len(lines)
    it = iter(out)
    for nd, st, want_st, want_nu in THINNING:
        assert [int(v) for v in next(it).split()] == [want_st, want_nu] == list(sc.thinning(nd, st)) == list(_lib.score_thinning(nd, st))
    for nT in pairings:
        got = [[int(r) for r in blk.split(",")] for blk in next(it).strip(";").split(";")]
        assert got == sc.row_pairing(nT)
        assert sorted(r for blk in got for r in blk) == list(range(nT))                      # every row of tiles exactly once
        pairs = [(r, J) for blk in got for r in blk for J in range(r + 1)]
        assert sorted(pairs) == [(r, J) for r in range(nT) for J in range(r + 1)]           # so every tile pair J <= r exactly once
        load = [sum(r + 1 for r in blk) for blk in got]
        assert all(x == nT + 1 for x in load[:nT // 2]) and (nT % 2 == 0 or load[-1] == (nT + 1) // 2)
    for n_u, K, n_h in works:
        v = [int(x) for x in next(it).split()]
        N = n_u * K
        assert v[:3] == [0, N, 2 * N] and v[3] == (2 + n_h) * N and v[4] == v[3] + 3 * n_h * (-(-n_u // 1024))
        assert v[5] == sc.work_doubles(n_u, K, n_h) == v[4] + n_h * sc.blocks(N) and v[6] == 3 * v[5]
    for W, n_u, ncol, cap in groups:
        g = (64 << 20) // (8 * ncol * n_u)
        g = min(g, cap) if cap > 0 else g
        assert int(next(it)) == min(W, max(1, g))
    for m, s in avals:
        got = _unhex(next(it))
        want = float(sc.a_ld(np.array(m), np.array(s)))
        if s == 0.0:
            assert got == abs(m)                              # the one special case, exact
        elif not np.isfinite(want):
            assert (np.isnan(got) and np.isnan(want)) or got == want, (m, s)
        else:
            assert abs(got - want) <= sc.C_TERM * 2.0 ** -52 * want and got >= max(abs(m), 0.79 * math.sqrt(s)) * (1 - 1e-15), (m, s, got, want)


def _one(K, nd, seed, horizons=(0,), round5=False, spread=1.0):
    return fc.make_draws(seed, 1, K, nd, 0, max(horizons) > 0, spread)


def test_reference_single_normal_is_the_closed_form():
    """K = 2 with both states the same normal, every draw alike: the mixture is that normal, whatever the weights."""
    for mean, var, y in ((1.5, 0.64, 2.0), (-3.0, 2.25, -3.0), (0.0, 1.0, 7.5)):
        mu, sig2 = np.full((1, 2, 5), mean), np.full((1, 2, 5), var)
        pi = np.tile(np.array([[0.25], [0.75]]), (1, 1, 5))
        ref, _ = sc.reference(mu, sig2, pi, None, np.array([[y]]), (0,), 1, False)
        want = sc.crps_normal(y, mean, math.sqrt(var))
        assert abs(ref[0, 0, 0] - want) <= 4 * np.spacing(max(want, ref[0, 0, 1])), (ref, want)
        assert abs(ref[0, 0, 2] - 2.0 * math.sqrt(var) / math.sqrt(math.pi)) <= 4 * np.spacing(ref[0, 0, 2])       # the Gini mean difference
        z = (y - mean) / math.sqrt(var)
        assert abs(ref[0, 0, 3] - 0.5 * math.erfc(-z / math.sqrt(2.0))) <= 2.0 ** -50
        assert abs(ref[0, 0, 4] - math.exp(-0.5 * z * z) / math.sqrt(2 * math.pi * var)) <= 2.0 ** -50


def test_reference_pair_form_is_the_integral():
    """CRPS = int (F(x) - 1{x >= y})^2 dx: the pair form against a long-double trapezoid built on fan_cases.Fld (K = 3, 300
    draws), cut at y where the integrand jumps; the trapezoid's own error is bounded by what halving the step moves it."""
    K, nd, y = 3, 300, 2.7
    mu, sig2, pi, _ = _one(K, nd, 41)
    ref, bound = sc.reference(mu, sig2, pi, None, np.array([[y]]), (0,), 1, False)
    wts = fc.omega(pi[0], None, 0, LD)
    # 9 standard deviations past every mean: beyond them F (1 - F) is below 1e-18, so the cut tails are far below the bound
    lo, hi = float(np.min(mu[0] - 9.0 * np.sqrt(sig2[0]))), float(np.max(mu[0] + 9.0 * np.sqrt(sig2[0])))

    P = 1 << 13
    coarse, fine = LD(0.0), LD(0.0)
    for a, b, up in ((lo, y, False), (y, hi, True)):
        x = np.linspace(LD(a), LD(b), P + 1, dtype=LD)
        F = fc.Fld(x, mu[0], sig2[0], wts)
        g = (1 - F) ** 2 if up else F ** 2
        fine = fine + ((g[:-1] + g[1:]).sum() / 2) * (LD(b) - LD(a)) / P
        g = g[::2]                                                                          # the same rule at twice the step
        coarse = coarse + ((g[:-1] + g[1:]).sum() / 2) * (LD(b) - LD(a)) / (P // 2)
    err = abs(float(coarse - fine))
    print("crps %.12g, trapezoid %.12g, halving moved it by %.3g" % (ref[0, 0, 0], float(fine), err))
    assert err < 1e-5 * ref[0, 0, 0]                                                        # the quadrature has converged
    assert abs(ref[0, 0, 0] - float(fine)) <= err + bound[0, 0, 0]


@pytest.mark.parametrize("K,nd,horizons,round5", [(2, 150, (0,), True), (3, 200, (0, 1, 12), True), (8, 40, sc.H8, False)])
def test_reference_properties(K, nd, horizons, round5):
    """crps >= 0 and below e_abs; pit is the CDF of the float64 restatement within the CDF entry's bound; the scores do not
    depend on the order of the draws nor on the order of the labels within a draw, within the bound; equal horizons agree; a
    NaN yreal leaves e_pair alone."""
    mu, sig2, pi, A = _one(K, nd, 50 + K, horizons, round5)
    rng = np.random.default_rng(K)
    y = rng.normal(2.0, 3.0, size=(len(horizons), 1))
    ref, bound = sc.reference(mu, sig2, pi, A, y, horizons, 1, round5)
    assert (ref[..., 0] >= 0.0).all() and (ref[..., 0] <= ref[..., 1]).all() and (ref[..., 2] > 0.0).all()
    assert ((ref[..., 3] >= 0.0) & (ref[..., 3] <= 1.0 + 1e-4)).all() and (ref[..., 4] > 0.0).all()
    rd = fc._rd(round5)
    for j, h in enumerate(horizons):
        w64 = fc.omega(rd(pi[0]), rd(A[0]) if h > 0 else None, h)
        F = fc.F64(np.array([y[j, 0]]), rd(mu[0]), rd(sig2[0]), w64)[0]
        assert abs(F - ref[0, j, 3]) <= pc.tolerance(nd, K, max(horizons))
    perm = rng.permutation(nd)
    lab = rng.permutation(K)
    mu2, sig22, pi2 = mu[:, lab][:, :, perm], sig2[:, lab][:, :, perm], pi[:, lab][:, :, perm]
    A2 = A[:, lab][:, :, lab][:, :, :, perm] if A is not None else None
    ref2, _ = sc.reference(mu2, sig22, pi2, A2, y, horizons, 1, round5)
    assert sc.worst_ratio(ref2, ref, bound) <= 1.0
    if horizons.count(0) > 1:
        assert ref[0, 0, 2] == ref[0, 1, 2]                                # the realised values differ; e_pair is the horizon's alone
    y[0, 0] = np.nan
    ref3, _ = sc.reference(mu, sig2, pi, A, y, horizons, 1, round5)
    assert np.isnan(ref3[0, 0, [0, 1, 3, 4]]).all() and np.array_equal(ref3[..., 2], ref[..., 2]) and np.array_equal(ref3[0, 1:], ref[0, 1:])


def test_reference_zero_variance_rule():
    """a(0, 0) = 0 and a(m, 0) = |m|: a point mass at mu scores |y - mu|, its Gini mean difference is 0; two point masses score
    by the discrete formula."""
    assert float(sc.a_ld(np.array(0.0), np.array(0.0))) == 0.0 and float(sc.a_ld(np.array(-1.75), np.array(0.0))) == 1.75
    mu, sig2 = np.full((1, 2, 3), 1.25), np.zeros((1, 2, 3))
    pi = np.full((1, 2, 3), 0.5)
    ref, _ = sc.reference(mu, sig2, pi, None, np.array([[3.0]]), (0,), 1, False)
    assert ref[0, 0, 0] == 1.75 and ref[0, 0, 1] == 1.75 and ref[0, 0, 2] == 0.0
    mu[0, 1] = 2.25                                                                        # masses at 1.25 and 2.25, half each
    ref, _ = sc.reference(mu, sig2, pi, None, np.array([[3.0]]), (0,), 1, False)
    assert ref[0, 0, 1] == 1.25 and ref[0, 0, 2] == 0.5 and ref[0, 0, 0] == 1.0


def _hand_made(seed, K=3, n=300):
    """Draws in the reference's Julia shapes: means, variances, states (n, K), A (n, K, K) with A[d, i, j]."""
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((n, K)) + 3.0 * np.arange(K)
    variances = 0.05 + rng.gamma(2.0, 0.8, size=(n, K))
    states = rng.dirichlet(np.ones(K), size=n)
    A = 0.1 * rng.dirichlet(np.ones(K) * 2.0, size=(n, K)) + 0.9 * np.eye(K)
    return means, variances, states, A


def test_calcscores_file_route_writer_and_summary(tmp_path):
    """Per-draw files written by hmc.saveresults from hand-made draws (K = 3, n = 300, two dates) through hmc.calcscores (float64
    numpy, no GPU) against the reference on the same draws rounded as the cells are, within the bound (the file route sums in
    float64 in numpy's order: the same bound covers it, its chains are no longer); thinned and exact; then the writer's text
    and the summary."""
    dates = [dt.date(1980, 1, 1), dt.date(1985, 1, 1)]
    draws = [_hand_made(81 + i) for i in range(2)]
    for d, (means, variances, states, A) in zip(dates, draws):
        n, K = means.shape
        ds = [dt.date(1960 + i // 12, i % 12 + 1, 1) for i in range(11)] + [d]
        opt = hmc.estopt(np.zeros(12), ds, sampleRange=range(1, 13), endIndex=12, horizons=(12,), D=K, burnin=1, Nrun=n)
        hmc.saveresults(hmc.Samples(means, variances, states[:, None, :], A, np.zeros((n, 2)), [d] * n), opt, str(tmp_path), native=False)
    mu, sig2 = np.stack([m.T for m, _, _, _ in draws]), np.stack([v.T for _, v, _, _ in draws])
    pi = np.stack([s.T for _, _, s, _ in draws])
    A = np.stack([np.transpose(a, (2, 1, 0)) for _, _, _, a in draws])
    horizons = (0, 12)
    yreal = np.array([[2.5, np.nan], [4.0, -1.0]])                                          # (dates, horizons)
    for stride in (1, 7):
        got_dates, s = hmc.calcscores(str(tmp_path), dates, horizons, yreal, stride=stride)
        assert got_dates == [str(x) for x in dates] and s["crps"].shape == (2, 2) and s["stride"] == stride and s["horizons"] == horizons
        ref, bound = sc.reference(mu, sig2, pi, A, yreal.T, horizons, stride, True)
        got = np.stack([s[name] for name in _lib.SCORE_FIELDS], axis=-1)
        worst = sc.worst_ratio(got, ref, bound)
        print("file route, stride %d: max |files - ref| / bound = %.3g" % (stride, worst))
        assert worst <= 1.0
        assert np.isnan(s["crps"][0, 1]) and np.isfinite(s["e_pair"]).all() and np.array_equal(np.isnan(s["yreal"]), np.isnan(yreal))
    with pytest.raises(FileNotFoundError):
        hmc.calcscores(str(tmp_path), [dt.date(1990, 1, 1)], (0,), [[0.0]])
    with pytest.raises(ValueError, match="stride >= 0"):
        hmc.calcscores(str(tmp_path), dates, (0,), np.zeros((2, 1)), stride=-1)
    path = hmc.write_scores(str(tmp_path / "scores.csv"), got_dates, s)
    header, rows = hmc._read_csv(path)
    assert header == ["date", "horizon", "yreal", "crps", "e_abs", "e_pair", "pit", "pdf"] and len(rows) == 4
    assert rows[1][:4] == ["1980-01-01", "12", "NaN", "NaN"] and rows[1][5] == hmc._fmt(s["e_pair"][0, 1])
    assert rows[2] == ["1985-01-01", "0", "4"] + [hmc._fmt(s[name][1, 0]) for name in _lib.SCORE_FIELDS]
    back = np.array([[float(x) for x in r[3:]] for r in rows]).reshape(2, 2, 5)             # shortest round-trip text: the same doubles
    assert np.array_equal(back, got, equal_nan=True)
    sm = hmc.scoresummary(s)
    assert list(sm["count"]) == [2, 1] and sm["mean_crps"][0] == (s["crps"][0, 0] + s["crps"][1, 0]) / 2 and sm["mean_crps"][1] == s["crps"][1, 1]
    assert sm["pit_hist"].shape == (2, 10) and list(sm["pit_hist"].sum(axis=1)) == [2, 1]


def test_scoresummary_on_a_hand_made_table():
    crps = np.array([[0.5, np.nan], [1.5, 2.0], [1.0, 4.0], [np.nan, np.nan]])
    pit = np.array([[0.05, np.nan], [0.95, 1.0], [0.5, 0.0], [np.nan, np.nan]])
    sm = hmc.scoresummary({"crps": crps, "pit": pit})
    assert list(sm["count"]) == [3, 2] and list(sm["mean_crps"]) == [1.0, 3.0]
    assert list(sm["pit_hist"][0]) == [1, 0, 0, 0, 0, 1, 0, 0, 0, 1] and list(sm["pit_hist"][1]) == [1, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    none = hmc.scoresummary({"crps": np.full((2, 1), np.nan), "pit": np.full((2, 1), np.nan)})
    assert list(none["count"]) == [0] and np.isnan(none["mean_crps"][0]) and none["pit_hist"].sum() == 0


def test_batchresult_scores_is_none_unless_asked_for():
    res = hmc.BatchResult([], {"summary": np.zeros((0, 1)), "status": np.zeros(0, dtype=np.int32)}, False)
    assert res.scores is None
    with pytest.raises(ValueError, match="no scores"):
        hmc.calcscores("unused", ["1980-01-01"], (0,), None, result=res)
