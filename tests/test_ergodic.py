"""Ergodic regime law, durations and long-run moments of the draws (hmcg_ergodic_moments[_device], include/hmcg_ergodic.h)
without a GPU: the ABI against the header, every misuse rule from the built library, csrc/ergodic_plan.hpp run on the CPU (plain
and under sanitizers) against the numpy restatement bit for bit, the restatement against its longdouble twin within the derived
bounds where a linear solve is far outside them, and the file route of hmc.calcergodic with its writer."""
import ctypes as C
import datetime as dt
import os
import subprocess

import numpy as np
import pytest

import hmc_jl_amd
from hmc_jl_amd import _lib, hmc

import ergodic_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERGODIC = _lib.Ergodic                # the whole module is about this feature: without the binding none of it runs
ENTRIES = ["hmcg_ergodic_moments", "hmcg_ergodic_moments_device"]


def test_ctypes_struct_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%%zu %%zu %%zu %%zu %%zu %%d %%d %%d %%d", '
                   'sizeof(hmcg_ergodic), offsetof(hmcg_ergodic, nd), offsetof(hmcg_ergodic, nd_ld), offsetof(hmcg_ergodic, flags), '
                   'offsetof(hmcg_ergodic, reserved), HMCG_ERG_ROUND5, HMCG_ERG_COLS(2), HMCG_ERG_COLS(8), HMCG_VERSION);return 0;}\n'
                   % os.path.join(ROOT, "include", "hmcg_ergodic.h"))
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    E = ERGODIC
    assert got[:5] == [C.sizeof(E), E.nd.offset, E.nd_ld.offset, E.flags.offset, E.reserved.offset] and C.sizeof(E) == 40
    assert got[5:8] == [_lib.ERG_ROUND5, _lib.erg_cols(2), _lib.erg_cols(8)] == [1, 6, 18]
    lib = hmc_jl_amd.load()
    assert got[8] == 109 == lib.hmcg_version()                 # a companion header: the version stays
    assert _lib.ERGODIC_EXPORTS == ("hmcg_ergodic_moments", "hmcg_ergodic_moments_device")
    assert not set(_lib.ERGODIC_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.ORDER_EXPORTS))
    for name in _lib.ERGODIC_EXPORTS:
        assert getattr(lib, name).restype is C.c_int
    assert len(_lib.erg_names(3)) == _lib.erg_cols(3) == ec.ncols(3)


def test_symbols_are_exported_by_the_built_library():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH]).decode()
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(_lib.ERGODIC_EXPORTS) <= names


# In the header's order.  Fields overwritten on a good call | pointers withheld | text of the refusal.
MISUSE = [
    (dict(struct_size=7), {}, b"hmcg_ergodic.struct_size 7 != 40"),
    (dict(K=1), {}, b"K = 1 outside 2..8"),
    (dict(K=9), {}, b"K = 9 outside 2..8"),
    (dict(W=0), {}, b"W = 0: at least one window"),
    (dict(nd=0, nd_ld=0), {}, b"nd = 0: at least one draw"),
    (dict(nd_ld=39), {}, b"nd_ld = 39 < nd = 40"),
    ({}, dict(mu=False), b"required"),
    ({}, dict(sig2=False), b"required"),
    ({}, dict(A=False), b"required"),
    ({}, dict(out=False), b"required"),
    ({}, dict(n=False), b"required"),
]
# Two rules broken at once: the rule the header names first.
DOUBLY_WRONG = [
    (dict(struct_size=7, K=1), {}, b"hmcg_ergodic.struct_size 7 != 40"),
    (dict(K=9, W=0), {}, b"K = 9 outside 2..8"),
    (dict(W=0, nd=0), {}, b"W = 0: at least one window"),
    (dict(nd=0, nd_ld=-1), {}, b"nd = 0: at least one draw"),
    (dict(nd_ld=39), dict(mu=False), b"nd_ld = 39 < nd = 40"),
]


def _call(lib, entry, p, ptrs):
    buf = np.zeros(64)
    ok = C.c_void_p(buf.ctypes.data)
    a = [ok if ptrs.get(n, True) else None for n in ("mu", "sig2", "A", "cols", "out", "n")]
    return getattr(lib, entry)(p, *(a + ([None] if entry.endswith("device") else []) + [None]))


@pytest.mark.parametrize("entry", ENTRIES)
def test_misuse_is_refused_before_device_init(entry):
    """Every rule returns HMCG_E_BADARG with its text from the built library; the data pointers are never followed (the device
    entry is handed host addresses here) and no GPU is needed: the check precedes get_context.  cols may be NULL: withholding
    it is no misuse, so a call that is wrong elsewhere is refused for that reason with or without it."""
    lib = hmc_jl_amd.load()
    for fields, ptrs, text in MISUSE + DOUBLY_WRONG:
        for with_cols in (True, False):
            p = _lib.make_ergodic(1, 3, 40, 40)
            for k, v in fields.items():
                setattr(p, k, v)
            rc = _call(lib, entry, C.byref(p), dict(ptrs, cols=with_cols))
            assert rc == -1 and text in lib.hmcg_last_error(), (fields, ptrs, rc, lib.hmcg_last_error())
    assert _call(lib, entry, None, {}) == -1 and b"hmcg_ergodic is NULL" in lib.hmcg_last_error()
    with pytest.raises(ValueError, match="A is required"):
        _lib.ergodic_moments(np.zeros((1, 3, 4)), np.zeros((1, 3, 4)), None)
    with pytest.raises(ValueError, match="A must have the shape"):
        _lib.ergodic_moments(np.zeros((1, 3, 4)), np.zeros((1, 3, 4)), np.zeros((1, 3, 2, 4)))


PLAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "%s"
using namespace hmcg_host;
// one line of stdin per draw: K, then K * K cells of A in the ABI's order (i fastest; the diagonal cells are given and never
// read), K of mu, K of sig2, each as 16 hex digits; one line of stdout per draw: the 2K + 2 columns as 16 hex digits
template <int K>
static void one(const double* in)
{
    double P[K * K], mu[K], s2[K], o[2 * K + 2];
    memcpy(P, in, sizeof P);
    memcpy(mu, in + K * K, sizeof mu);
    memcpy(s2, in + K * K + K, sizeof s2);
    erg_draw<K>(P, mu, s2, o);
    for (int c = 0; c < 2 * K + 2; ++c) {
        unsigned long long u;
        memcpy(&u, &o[c], 8);
        std::printf("%%016llx%%c", u, c == 2 * K + 1 ? '\n' : ' ');
    }
}
int main()
{
    for (int K = 2; K <= HMCG_MAXK; ++K)
        std::printf("%%d %%d %%d %%zu%%c", erg_cols(K), erg_items(K), erg_columns(K), erg_part_doubles(3, 2051, K), K == HMCG_MAXK ? '\n' : ' ');
    int K;
    while (std::scanf("%%d", &K) == 1) {
        double in[HMCG_MAXK * HMCG_MAXK + 2 * HMCG_MAXK];
        for (int q = 0; q < K * K + 2 * K; ++q) {
            unsigned long long u;
            if (std::scanf("%%llx", &u) != 1) return 2;
            memcpy(&in[q], &u, 8);
        }
        switch (K) {
            case 2: one<2>(in); break;
            case 3: one<3>(in); break;
            case 4: one<4>(in); break;
            case 5: one<5>(in); break;
            case 6: one<6>(in); break;
            case 7: one<7>(in); break;
            case 8: one<8>(in); break;
            default: return 3;
        }
    }
    return 0;
}
"""


def _hex(x):
    return "%016x" % int(np.float64(x).view(np.uint64))


def _directed_draws():
    """(K, A (K, K) in the ABI's order [j, i], mu, sig2) of every directed kind for K = 2..8, and a few generic persistent ones."""
    out = []
    for K in ec.KS:
        rng = np.random.default_rng(40 + K)
        for name in ec.DIRECTED:
            a, m, s = ec.directed(name, K, rng)
            out.append((name, K, np.ascontiguousarray(a.T), m, s))
        mu, sig2, A = ec.make_panel(7 * K, 1, K, 6)
        for d in range(6):
            out.append(("generic", K, A[0, :, :, d].copy(), mu[0, :, d].copy(), sig2[0, :, d].copy()))
    return out


def test_plan_header_on_the_cpu(tmp_path):
    """csrc/ergodic_plan.hpp, compiled by g++ -Wall -Werror into a stand-alone program and once more with
    -fsanitize=address,undefined (nothing is loaded into Python): erg_draw<K> for K = 2..8 on the directed matrices prints the
    bits of the numpy restatement -- the statements the kernel compiles -- and the directed kinds give what their names say."""
    src = tmp_path / "plan_main.cpp"
    src.write_text(PLAN_MAIN % os.path.join(ROOT, "hmc.jl_amd", "csrc", "ergodic_plan.hpp"))
    exe, san = tmp_path / "plan_main", tmp_path / "plan_main_san"
    flags = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror"]
    subprocess.check_call(flags + [str(src), "-o", str(exe)])
    subprocess.check_call(flags + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", str(src), "-o", str(san)])
    draws = _directed_draws()
    text = "".join("%d %s\n" % (K, " ".join(_hex(v) for v in list(a.reshape(-1)) + list(m) + list(s))) for _, K, a, m, s in draws)
    out = subprocess.run([str(exe)], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    assert subprocess.run([str(san)], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines() == out
    sizes = [int(v) for v in out[0].split()]
    for i, K in enumerate(ec.KS):                                # columns, slab sums, upload columns, the work area of W = 3, 3 slabs
        assert sizes[4 * i:4 * i + 4] == [2 * K + 2, 4 * K + 5, K * K + 2 * K, 3 * (3 * (4 * K + 5) + 2 * K + 2)]
    assert len(out) == 1 + len(draws)
    for line, (name, K, a, m, s) in zip(out[1:], draws):
        got = np.array([int(h, 16) for h in line.split()], dtype=np.uint64).view(np.float64)
        want = ec.columns(m[:, None], s[:, None], a[:, :, None])[:, 0]
        assert ec.same_cells(got, want), (name, K, got, want)
        assert np.isfinite(got).all() == ec.directed_good(name, K), (name, K, got)
        pi, dur = got[:K], got[K:2 * K]
        if name == "absorbing first":
            assert np.array_equal(pi, np.eye(K)[0]) and dur[0] == np.inf and np.isfinite(dur[1:]).all()
        if name == "absorbing last":
            assert not np.isfinite(pi).all() and dur[K - 1] == np.inf
        if name == "transient":
            assert pi[K - 1] == 0.0 and not np.signbit(pi[K - 1]) and (pi[:K - 1] > 0.0).all()
        if name == "persistent":                                 # a cycle: the uniform law to a few roundings, durations 1e5
            assert np.allclose(pi, 1.0 / K, rtol=1e-14, atol=0.0) and (dur == 1.0 / 1e-5).all()
        if name == "equal mu":
            tol = ec.gamma(ec.depth(K)[0] + K) * abs(m[0])          # m = mu_0 sum_k pi_k, the sum 1 to its rounding count
            assert abs(got[2 * K] - m[0]) <= tol and abs(got[2 * K + 1] - (got[:K] * s).sum()) <= 4.0 * tol * tol + K * ec.U * got[2 * K + 1]
        if name == "sig2 zero":
            assert got[2 * K + 1] >= 0.0


def test_nan_diagonal_changes_nothing():
    for K in ec.KS:
        mu, sig2, A = ec.make_panel(K, 1, K, 64)
        B = A.copy()
        B[0, np.arange(K), np.arange(K), :] = 0.25
        assert ec.same_cells(ec.panel_columns(mu, sig2, A), ec.panel_columns(mu, sig2, B))


@pytest.mark.parametrize("K", ec.KS)
def test_restatement_within_the_derived_bounds_where_a_solve_is_not(K):
    """3 000 rounded, nearly reducible matrices: the float64 restatement is within ergodic_cases.column_bounds of its longdouble
    twin in every column, exact zeros and non-finite cells in the same places -- and numpy.linalg.solve on the same matrices
    misses the bound on pi by orders of magnitude, which is why the library eliminates without subtracting."""
    n = 3000
    Ad = ec.nearly_reducible(K, n, K)
    A = ec.to_abi(Ad)
    rng = np.random.default_rng(100 + K)
    mu = rng.standard_normal((K, n)) + 2.0 * np.arange(K)[:, None]
    sig2 = rng.gamma(2.0, 0.8, size=(K, n))
    got, ref = ec.columns(mu, sig2, A), ec.columns(mu, sig2, A, ec.LD)
    rf = ref.astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(rf)) and np.array_equal(np.isinf(got), np.isinf(rf))
    assert np.array_equal(got == 0.0, rf == 0.0)
    fin = np.isfinite(rf)
    bound = ec.column_bounds(ref, mu, sig2)
    diff = np.where(fin, np.abs(np.where(fin, got, 0.0).astype(ec.LD) - np.where(fin, ref, 0.0)), 0.0).astype(np.float64)
    assert (diff <= bound).all(), float(np.max(diff / np.where(bound > 0.0, bound, 1.0)))
    c_pi, c_dur = ec.depth(K)
    good = np.flatnonzero(fin.all(axis=0))
    assert good.size > n // 2
    worst_solve = worst_gth = 0.0
    for d in good:
        q = rf[:K, d]
        nz = q > 0.0
        try:
            s = ec.solve_pi(Ad[d])
        except np.linalg.LinAlgError:
            continue
        worst_solve = max(worst_solve, float(np.max(np.abs(s[nz] - q[nz]) / q[nz])))
        worst_gth = max(worst_gth, float(np.max(np.abs(got[:K, d][nz] - q[nz]) / q[nz])))
    print("K = %d: rounding counts pi %d, dur %d; GTH %.1f u, solve %.3g u, bound %.0f u" %
          (K, c_pi, c_dur, worst_gth / ec.U, worst_solve / ec.U, ec.gamma(c_pi) / ec.U))
    assert worst_gth <= ec.gamma(c_pi) * ec.REF < worst_solve


def _hand_made(seed, K=3, n=300):
    """Draws in the reference's Julia shapes: means, variances, states (n, K), A (n, K, K) with A[d, i, j]; persistent rows, one
    draw with an absorbing state."""
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((n, K)) + 3.0 * np.arange(K)
    variances = 0.05 + rng.gamma(2.0, 0.8, size=(n, K))
    states = rng.dirichlet(np.ones(K), size=n)
    A = 0.03 * rng.dirichlet(np.ones(K) * 2.0, size=(n, K)) + 0.97 * np.eye(K)
    A[7, 1] = np.eye(K)[1]
    return means, variances, states, A


def test_calcergodic_file_route_and_writer(tmp_path):
    """Per-draw files written by hmc.saveresults from hand-made draws (K = 3, n = 300, two dates) through hmc.calcergodic
    (numpy, no GPU): its per-draw columns are the restatement's on the same draws rounded as the cells are, bit for bit; its
    pooled moments within the derived bound of the longdouble moments of those columns; then the writer's text."""
    dates = [dt.date(1980, 1, 1), dt.date(1985, 1, 1)]
    draws = [_hand_made(61 + i) for i in range(2)]
    for d, (means, variances, states, A) in zip(dates, draws):
        n, K = means.shape
        ds = [dt.date(1960 + i // 12, i % 12 + 1, 1) for i in range(11)] + [d]
        opt = hmc.estopt(np.zeros(12), ds, sampleRange=range(1, 13), endIndex=12, horizons=(12,), D=K, burnin=1, Nrun=n)
        hmc.saveresults(hmc.Samples(means, variances, states[:, None, :], A, np.zeros((n, 2)), [d] * n), opt, str(tmp_path), native=False)
    mu, sig2 = np.stack([m.T for m, _, _, _ in draws]), np.stack([v.T for _, v, _, _ in draws])
    A = np.stack([np.transpose(a, (2, 1, 0)) for _, _, _, a in draws])
    got_dates, e = hmc.calcergodic(str(tmp_path), dates, cols=True)
    assert got_dates == [str(x) for x in dates] and e["cols"].shape == (2, 8, 300)
    assert ec.same_cells(e["cols"], ec.panel_columns(mu, sig2, A, round5_=True))
    assert (e["good"] == 299).all() and (e["bad"] == 1).all() and e["cols"][0, 3 + 1, 7] == np.inf
    out = np.stack([np.concatenate([e["pi_" + k], e["dur_" + k], e["mean_" + k][:, None], e["variance_" + k][:, None]], axis=1)
                    for k in ("mean", "var")], axis=2)
    ec.check_pooled(out, np.stack([e["good"], e["bad"]], axis=1), e["cols"], "files")
    assert np.allclose(e["pi_mean"].sum(axis=1), 1.0, atol=1e-12) and (e["dur_mean"] > 10.0).all()
    assert "cols" not in hmc.calcergodic(str(tmp_path), dates)[1]
    with pytest.raises(FileNotFoundError):
        hmc.calcergodic(str(tmp_path), [dt.date(1990, 1, 1)])
    path = hmc.write_ergodic(str(tmp_path / "ergodic.csv"), got_dates, e)
    header, rows = hmc._read_csv(path)
    assert header == ["date", "column", "mean", "variance", "good", "bad"] and len(rows) == 2 * 8
    assert [r[1] for r in rows[:8]] == ["pi1", "pi2", "pi3", "dur1", "dur2", "dur3", "mean", "variance"]
    r = rows[8 + 6]
    assert r == ["1985-01-01", "mean", hmc._fmt(e["mean_mean"][1]), hmc._fmt(e["mean_var"][1]), "299", "1"]


def test_batchresult_ergodic_is_none_unless_asked_for():
    res = hmc.BatchResult([], {"summary": np.zeros((0, 1)), "status": np.zeros(0, dtype=np.int32)}, False)
    assert res.ergodic is None
    with pytest.raises(ValueError, match="no ergodic moments"):
        hmc.calcergodic("unused", ["1980-01-01"], result=res)
