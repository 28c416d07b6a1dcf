"""Predictive CDFs of the regime mixture (hmcg_predictive_cdf, calc_cdfs.jl): the parts that need no GPU -- the struct and the
argument rules of the built library (checked before device init), the slab / chunk cut of csrc/stat_plan.hpp (through
predictive_plan.hpp) run by a g++-compiled program, and the host-side file route of hmc.calccdfs against the direct formula."""
import ctypes as C
import datetime as dt
import math
import os
import subprocess

import numpy as np
import pytest

import hmc_jl_amd
from hmc_jl_amd import _lib, hmc

import predictive_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ctypes_struct_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "%s"\nint main(void){printf("%%zu %%d %%d %%d", sizeof(hmcg_predictive), '
                   'HMCG_MAXGRID, HMCG_PRED_MAXH, HMCG_PRED_ROUND5);return 0;}\n' % os.path.join(ROOT, "include", "hmcg.h"))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.Predictive), _lib.HMCG_MAXGRID, _lib.HMCG_PRED_MAXH, _lib.PRED_ROUND5]


MISUSE = [
    (dict(struct_size=7), {}, b"struct_size"),
    (dict(K=1), {}, b"K = 1"),
    (dict(K=9), {}, b"K = 9"),
    (dict(G=0), {}, b"grid points"),
    (dict(G=_lib.HMCG_MAXGRID + 1), {}, b"grid points"),
    (dict(n_h=0), {}, b"horizons outside"),
    (dict(n_h=_lib.HMCG_MAXH + 1), {}, b"horizons outside"),
    (dict(h0=-1), {}, b"horizon -1"),
    (dict(h0=_lib.HMCG_PRED_MAXH + 1), dict(A=True), b"horizon 1025"),
    (dict(nd=0), {}, b"at least one draw"),
    (dict(nd_ld=3), {}, b"nd_ld"),
    ({}, dict(mu=False), b"required"),
    ({}, dict(sig2=False), b"required"),
    ({}, dict(pi_end=False), b"required"),
    ({}, dict(grid=False), b"required"),
    ({}, dict(cdf=False), b"required"),
    (dict(h0=2), {}, b"A is NULL"),
]


@pytest.mark.parametrize("entry", ["hmcg_predictive_cdf", "hmcg_predictive_cdf_device"])
def test_misuse_is_refused_before_device_init(entry):
    """Every rule returns HMCG_E_BADARG with its text from the built library; the pointers are never followed (the device entry is
    handed host addresses here) and no GPU is needed: the check precedes get_context."""
    lib = hmc_jl_amd.load()
    buf = np.zeros(64)
    ok = C.c_void_p(buf.ctypes.data)
    for fields, ptrs, text in MISUSE:
        p = _lib.make_predictive(1, 3, 4, 4, 2, (0,))
        for k, v in fields.items():
            if k == "h0":
                p.horizons[0] = v
            else:
                setattr(p, k, v)
        a = {n: (ok if ptrs.get(n, n != "A") else None) for n in ("mu", "sig2", "pi_end", "A", "grid", "cdf")}
        fn = getattr(lib, entry)
        args = [C.byref(p), a["mu"], a["sig2"], a["pi_end"], a["A"], a["grid"], a["cdf"]] + ([None] if entry.endswith("device") else []) + [None]
        rc = fn(*args)
        assert rc == -1 and text in lib.hmcg_last_error(), (fields, ptrs, rc, lib.hmcg_last_error())


# Two rules broken at once: the rule the entry names first, with its whole text.  The order is this feature's own (G and the
# horizons stand between K and nd); the texts of the rules it shares with the other draw statistics come from csrc/stat_plan.hpp.
DOUBLY_WRONG = [
    (dict(struct_size=7, W=0), b"hmcg_predictive.struct_size 7 != %d" % C.sizeof(_lib.Predictive)),
    (dict(W=0, nd_ld=3), b"W = 0: at least one window"),
    (dict(K=9, nd=0), b"K = 9 outside 2..8"),
    (dict(G=0, nd=0), b"G = 0 grid points outside 1..4096"),
    (dict(n_h=0, nd=0), b"n_h = 0 horizons outside 1..8"),
    (dict(h0=-1, nd_ld=3), b"horizon -1 outside 0..1024"),
    (dict(nd=0, nd_ld=-1), b"nd = 0: at least one draw"),
    (dict(nd_ld=3, h0=2), b"nd_ld = 3 < nd = 4"),
]


@pytest.mark.parametrize("fields, message", DOUBLY_WRONG)
@pytest.mark.parametrize("entry", ["hmcg_predictive_cdf", "hmcg_predictive_cdf_device"])
def test_first_rule_named_for_a_doubly_wrong_call(entry, fields, message):
    lib = hmc_jl_amd.load()
    buf = np.zeros(64)
    ok = C.c_void_p(buf.ctypes.data)
    p = _lib.make_predictive(1, 3, 4, 4, 2, (0,))
    for k, v in fields.items():
        if k == "h0":
            p.horizons[0] = v
        else:
            setattr(p, k, v)
    rc = getattr(lib, entry)(C.byref(p), ok, ok, ok, None, ok, ok, *(([None] if entry.endswith("device") else []) + [None]))
    assert rc == -1 and lib.hmcg_last_error() == message


def test_host_entry_refuses_a_non_finite_grid():
    lib = hmc_jl_amd.load()
    buf = np.zeros(64)
    grid = np.array([0.0, np.inf])
    p = _lib.make_predictive(1, 3, 4, 4, 2, (0,))
    ok = C.c_void_p(buf.ctypes.data)
    rc = lib.hmcg_predictive_cdf(C.byref(p), ok, ok, ok, None, C.c_void_p(grid.ctypes.data), ok, None)
    assert rc == -1 and b"grid[1] is not finite" in lib.hmcg_last_error()
    with pytest.raises(ValueError):
        _lib.make_predictive(1, 3, 4, 4, 2, (0,) * (_lib.HMCG_MAXH + 1))


PLAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "%s"
int main(int argc, char** argv)
{
    using namespace hmcg_host;
    std::printf("%%lld\n", PRED_SLAB);
    for (int i = 1; i + 1 < argc; i += 2) {
        const long long nd = std::atoll(argv[i]), cap = std::atoll(argv[i + 1]);
        const long long cd = pred_chunk_draws(nd, 3, 9, cap);
        std::printf("%%lld %%lld %%lld %%lld :", nd, cap, pred_slabs(nd), cd);
        for (const PredChunk& c : pred_chunks(nd, cd)) std::printf(" %%lld+%%lld", c.d0, c.n);
        std::printf("\n");
    }
    hmcg_predictive p{};
    p.struct_size = (int32_t)sizeof p; p.W = 1; p.K = 3; p.nd = p.nd_ld = 5; p.G = 2; p.n_h = 2; p.horizons[1] = 7;
    char msg[160] = "";
    const double x[2] = {0.0, 1.0};
    std::printf("%%d %%d %%d\n", check_predictive(&p, x, x, x, x, x, x, true, msg, sizeof msg), pred_max_horizon(p), pred_columns(p));
    std::printf("%%d %%s\n", check_predictive(&p, x, x, x, nullptr, x, x, true, msg, sizeof msg), msg);
    return 0;
}
"""


def test_slab_and_chunk_layout(tmp_path):
    """csrc/predictive_plan.hpp and the cut it takes from stat_plan.hpp, compiled by g++ into a stand-alone program: chunks are
    whole slabs (the last one ends at nd), start on slab boundaries and cover [0, nd) exactly once, for draw counts around the
    slab size and caps that are no slab multiple; the cap is rounded UP to whole slabs."""
    S = _lib.PRED_SLAB
    src = tmp_path / "plan_main.cpp"
    src.write_text(PLAN_MAIN % os.path.join(ROOT, "hmc.jl_amd", "csrc", "predictive_plan.hpp"))
    exe = tmp_path / "plan_main"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", str(src), "-o", str(exe)])
    table = [(1, 0), (S - 1, 0), (S, 0), (S + 1, 0), (S + 1, 1), (2 * S + 17, S - 1), (2 * S + 17, S + 1), (5 * S + 3, 1500),
             (250000, 0), (250000, 10000), (7 * S, 2 * S), (3, 7)]
    out = subprocess.check_output([str(exe)] + [str(v) for row in table for v in row]).decode().splitlines()
    assert int(out[0]) == S
    for (nd, cap), line in zip(table, out[1:]):
        head, _, tail = line.partition(":")
        nd_, cap_, nslab, cd = [int(v) for v in head.split()]
        assert (nd_, cap_) == (nd, cap) and nslab == -(-nd // S)
        assert cd % S == 0 and cd >= S
        if cap > 0 and cap < nd:
            assert cd == -(-cap // S) * S                      # honoured, rounded up to a slab multiple
        chunks = [tuple(int(v) for v in c.split("+")) for c in tail.split()]
        pos = 0
        for i, (d0, n) in enumerate(chunks):
            assert d0 == pos and d0 % S == 0 and n >= 1
            assert n % S == 0 or i == len(chunks) - 1
            assert n <= cd
            pos += n
        assert pos == nd
    assert out[len(table) + 1].split() == ["0", "7", "18"]
    assert out[len(table) + 2].startswith("-1 A is NULL")


def _direct(means, vars_, pis, A, ys, h):
    """calc_cdfs.jl:39-41 written out draw by draw in plain Python floats."""
    n, K = means.shape
    out = np.zeros(len(ys))
    vals = np.empty((n, len(ys)))
    for i in range(n):
        w = list(pis[i])
        for _ in range(h):
            w = [sum(w[a] * A[i][a][b] for a in range(K)) for b in range(K)]
        for g, y in enumerate(ys):
            s = 0.0
            for k in range(K):
                sd = math.sqrt(vars_[i, k])
                d = y - means[i, k]
                z = (d / sd) if sd != 0.0 else (math.nan if d == 0.0 else math.copysign(math.inf, d))
                s += w[k] * (math.erfc(-z / math.sqrt(2.0)) / 2.0)
            vals[i, g] = s
    with np.errstate(invalid="ignore"):
        out = vals.mean(axis=0)
    return out


def test_calccdfs_file_route(tmp_path):
    """Hand-written per-draw files of two dates (K = 3, 40 draws, written by basicsave) through hmc.calccdfs against the direct
    formula on the cells.  The first date holds a variance cell of 0.0 whose state's mean is a grid point: that grid cell is NaN,
    the ones beside it finite (the state contributes exactly 0 or its whole weight)."""
    rng = np.random.default_rng(11)
    K, n = 3, 40
    dates = [dt.date(1980, 1, 1), dt.date(1985, 1, 1)]
    ys = np.arange(-5, 15.25, .25)
    horizons = (0, 3)
    h1 = ["state_%d" % i for i in range(1, K + 1)]
    h2 = ["trans_%d_%d" % (i, j) for j in range(1, K + 1) for i in range(1, K + 1)]
    cells = {}
    for di, d in enumerate(dates):
        means = np.round(np.sort(rng.normal(3.0, 2.5, size=(n, K)), axis=1), 5)
        vars_ = np.round(0.05 + rng.gamma(2.0, 0.8, size=(n, K)), 5)
        pis = np.round(rng.dirichlet(np.ones(K), size=n), 5)
        A = np.round(rng.dirichlet(np.ones(K), size=(n, K)), 5)                  # [d, i, j]
        if di == 0:
            means[7, 1], vars_[7, 1] = 2.25, 0.0                               # 2.25 is a grid point
        cells[str(d)] = (means, vars_, pis, A)
        for stem, data, hdr in (("filtered_means", means, h1), ("filtered_variances", vars_, h1), ("filtered_state_probs", pis, h1),
                                ("filtered_trans_probs", A.reshape(n, K * K, order="F"), h2)):
            hmc.basicsave(data, [d] * n, str(tmp_path / ("%s_%s.csv" % (stem, d))), hdr)
    got_dates, got_ys, bar, fin = hmc.calccdfs(str(tmp_path), dates, ys, horizons)
    assert got_dates == [str(d) for d in dates] and np.array_equal(got_ys, ys) and bar.shape == (2, 2, 81) == fin.shape
    for di, d in enumerate(got_dates):
        means, vars_, pis, A = cells[d]
        for j, h in enumerate(horizons):
            exp = _direct(means, vars_, pis, A, ys, h)
            assert np.array_equal(np.isnan(bar[di, j]), np.isnan(exp))
            ok = ~np.isnan(exp)
            assert np.abs(bar[di, j][ok] - exp[ok]).max() < (n + 64 + 2 * K * h) * 2.0 ** -52
    g0 = int(np.where(ys == 2.25)[0][0])
    assert np.isnan(bar[0, 0]).sum() == 1 and np.isnan(bar[0, 0, g0]) and np.isnan(fin[0, 0, g0])
    assert np.isfinite(bar[0, 0, g0 - 1]) and np.isfinite(bar[0, 0, g0 + 1]) and np.isfinite(bar[1]).all()
    # horizon 0 alone never opens the transition file
    os.remove(tmp_path / ("filtered_trans_probs_%s.csv" % dates[1]))
    _, _, bar0, _ = hmc.calccdfs(str(tmp_path), dates[1:], ys)
    assert np.array_equal(bar0[0, 0], bar[1, 0])
    with pytest.raises(FileNotFoundError):
        hmc.calccdfs(str(tmp_path), dates[1:], ys, (1,))
    # the same numbers as the tests' reference on the same cells (C-ABI layouts)
    means, vars_, pis, A = cells[str(dates[1])]
    ref = pc.reference(means.T[None], vars_.T[None], pis.T[None], np.transpose(A, (2, 1, 0))[None], ys, horizons, False)
    assert np.abs(ref[0] - bar[1]).max() < (n + 64 + 2 * K * 3) * 2.0 ** -52


def test_calccdfs_result_route_checks():
    class R:
        cdf = None
    with pytest.raises(ValueError, match="no predictive CDFs"):
        hmc.calccdfs("unused", ["1980-01-01"], result=R())


def test_finverse():
    f = hmc.finverse([0.0, 1.0, 0.5, float("nan"), 0.975])
    assert f[0] == -math.inf and f[1] == math.inf and f[2] == 0.0 and math.isnan(f[3])
    assert abs(f[4] - 1.959963984540054) < 1e-12
    assert hmc.finverse(np.full((2, 3), 0.5)).shape == (2, 3)


def test_write_cdfs(tmp_path):
    bar = np.array([[[0.0, 0.5, 1.0], [0.25, float("nan"), 2.4e-10]]])
    path = hmc.write_cdfs(str(tmp_path / "cdfs.csv"), ["1980-01-01"], [-5.0, 0.25, 15.0], (0, 12), bar)
    lines = open(path).read().splitlines()
    assert lines[0] == "date,horizon,y,cdf,finverse" and len(lines) == 7
    assert lines[1] == "1980-01-01,0,-5,0,-Inf"
    assert lines[2] == "1980-01-01,0,0.25,0.5,0"
    assert lines[3] == "1980-01-01,0,15,1,Inf"
    assert lines[4].startswith("1980-01-01,12,-5,0.25,-0.67448975")
    assert lines[5] == "1980-01-01,12,0.25,NaN,NaN"
    assert lines[6].startswith("1980-01-01,12,15,24e-11,-6.")
