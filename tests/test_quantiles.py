"""Exact quantiles of the draws (hmcg_chain_quantiles[_device], include/hmcg_order.h) without a GPU: the ABI against the
header, every misuse rule from the built library, csrc/order_plan.hpp run on the CPU (plain and under sanitizers), the numpy
reference against np.quantile, the file route of hmc.calcquantiles and its writer."""
import ctypes as C
import datetime as dt
import os
import subprocess

import numpy as np
import pytest

import hmc_jl_amd
from hmc_jl_amd import _lib, hmc

import quantile_cases as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUANTILES = _lib.Quantiles            # the whole module is about this feature: without the binding none of it runs
ENTRIES = ["hmcg_chain_quantiles", "hmcg_chain_quantiles_device"]


def test_ctypes_struct_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%%zu %%zu %%zu %%zu %%zu %%d %%d %%d %%lld %%d", '
                   'sizeof(hmcg_quantiles), offsetof(hmcg_quantiles, nd), offsetof(hmcg_quantiles, Q), offsetof(hmcg_quantiles, flags), '
                   'offsetof(hmcg_quantiles, probs), HMCG_ORD_ROUND5, HMCG_ORD_MAXQ, HMCG_ORD_STRIDE, HMCG_ORD_MAXND, HMCG_VERSION);return 0;}\n'
                   % os.path.join(ROOT, "include", "hmcg_order.h"))
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    Q = QUANTILES
    assert got[:5] == [C.sizeof(Q), Q.nd.offset, Q.Q.offset, Q.flags.offset, Q.probs.offset] and C.sizeof(Q) == 168
    assert got[5:9] == [_lib.ORD_ROUND5, _lib.ORD_MAXQ, _lib.ORD_STRIDE, 2 ** 31 - 1] == [1, 16, 4, 2147483647]
    lib = hmc_jl_amd.load()
    assert got[9] == 109 == lib.hmcg_version()                 # a companion header: the version stays
    assert _lib.ORDER_EXPORTS == ("hmcg_chain_quantiles", "hmcg_chain_quantiles_device")
    assert not set(_lib.ORDER_EXPORTS) & set(_lib.EXPORTS)
    for name in _lib.ORDER_EXPORTS:
        assert getattr(lib, name).restype is C.c_int
    assert _lib.ORD_FIELDS == qc.FIELDS == ("value", "lo", "hi", "g") and len(_lib.ORD_FIELDS) == _lib.ORD_STRIDE


def _probs(*v):
    return {"probs": v}


MISUSE = [
    (dict(struct_size=7), {}, b"struct_size"),
    (dict(W=0), {}, b"at least one window"),
    (dict(C=0), {}, b"C = 0"),
    (dict(C=65), {}, b"C = 65"),
    (dict(nd=0, nd_ld=0), {}, b"at least one draw"),
    (dict(nd=2 ** 31, nd_ld=2 ** 31), {}, b"nd = 2147483648 exceeds 2147483647"),
    (dict(nd_ld=39), {}, b"nd_ld = 39 < nd = 40"),
    (dict(Q=0), {}, b"Q = 0 probabilities outside 1..16"),
    (dict(Q=17), {}, b"Q = 17 probabilities outside 1..16"),
    (dict(probs=(0.5, float("nan"))), {}, b"probs[1] = nan"),
    (dict(probs=(-0.1,)), {}, b"probs[0] = -0.1"),
    (dict(probs=(0.0, 1.0, 1.0000001)), {}, b"probs[2] = 1.0000001"),
    (dict(W=2 ** 29, C=64), {}, b"W * C exceeds one launch"),
    ({}, dict(x=False), b"required"),
    ({}, dict(q=False), b"required"),
    ({}, dict(n=False), b"required"),
]


def _wrong(fields):
    """A good call with `fields` overwritten; probs sets Q too unless Q is given."""
    p = _lib.make_quantiles(1, 3, 40, 40, (0.05, 0.5, 0.95))
    if "probs" in fields:
        p.Q = len(fields["probs"])
        for i, x in enumerate(fields["probs"]):
            p.probs[i] = x
    for k, v in fields.items():
        if k != "probs":
            setattr(p, k, v)
    return p


@pytest.mark.parametrize("entry", ENTRIES)
def test_misuse_is_refused_before_device_init(entry):
    """Every rule returns HMCG_E_BADARG with its text from the built library; the data pointers are never followed (the device
    entry is handed host addresses here) and no GPU is needed: the check precedes get_context."""
    lib = hmc_jl_amd.load()
    buf = np.zeros(64)
    ok = C.c_void_p(buf.ctypes.data)
    device = entry.endswith("device")
    for fields, ptrs, text in MISUSE:
        p = _wrong(fields)
        a = [ok if ptrs.get(n, True) else None for n in ("x", "q", "n")]
        rc = getattr(lib, entry)(C.byref(p), *(a + ([None] if device else []) + [None]))
        assert rc == -1 and text in lib.hmcg_last_error(), (fields, ptrs, rc, lib.hmcg_last_error())
    rc = getattr(lib, entry)(None, ok, ok, ok, *(([None] if device else []) + [None]))
    assert rc == -1 and b"hmcg_quantiles is NULL" in lib.hmcg_last_error()
    with pytest.raises(ValueError, match="at most 16 probabilities"):
        _lib.make_quantiles(1, 3, 40, 40, tuple(np.linspace(0, 1, 17)))
    with pytest.raises(_lib.HmcgError, match=r"probs\[1\] = 2"):
        _lib.chain_quantiles(np.zeros((1, 3, 4)), (0.5, 2.0))


# Two rules broken at once: the rule the entry names first, with its whole text.  The order is the header's; the texts of the
# rules it shares with the other draw statistics come from csrc/stat_plan.hpp.
DOUBLY_WRONG = [
    (dict(struct_size=7, W=0), b"hmcg_quantiles.struct_size 7 != 168"),
    (dict(W=0, C=0), b"W = 0: at least one window"),
    (dict(C=65, nd=0), b"C = 65 columns outside 1..64"),
    (dict(nd=0, nd_ld=-1), b"nd = 0: at least one draw"),
    (dict(nd=2 ** 31, nd_ld=4), b"nd = 2147483648 exceeds 2147483647 (HMCG_ORD_MAXND): the counters are 32-bit"),
    (dict(nd_ld=39, Q=0), b"nd_ld = 39 < nd = 40"),
    (dict(Q=17, probs=(2.0,) * 16), b"Q = 17 probabilities outside 1..16"),
    (dict(probs=(0.5, -0.1, float("nan")), W=2 ** 29, C=64), b"probs[1] = -0.10000000000000001 outside [0, 1]"),
    (dict(W=2 ** 29, C=64), b"W * C exceeds one launch (2^31 - 1 blocks)"),
]


@pytest.mark.parametrize("fields, message", DOUBLY_WRONG)
@pytest.mark.parametrize("entry", ENTRIES)
def test_first_rule_named_for_a_doubly_wrong_call(entry, fields, message):
    lib = hmc_jl_amd.load()
    buf = np.zeros(64)
    ok = C.c_void_p(buf.ctypes.data)
    p = _wrong(fields)
    last = None if message.startswith(b"W * C") else ok         # ... and ahead of the NULL rule
    rc = getattr(lib, entry)(C.byref(p), ok, ok, last, *(([None] if entry.endswith("device") else []) + [None]))
    assert rc == -1 and lib.hmcg_last_error() == message


PLAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "%s"
using namespace hmcg_host;
static double dbl(unsigned long long u) { double x; memcpy(&x, &u, 8); return x; }
int main(int argc, char** argv)
{
    // the constants and the digit schedule
    std::printf("%%d %%d %%u %%d %%d\n", ORD_BITS, ORD_DIGITS, ORD_MASK, ORD_MAXT, ORD_CAP);
    for (int d = 0; d < ORD_DIGITS; ++d) std::printf("%%d ", ord_shift(d));
    std::printf("\n");
    // the key of every double given as 16 hex digits, its inverse's bits
    int a = 1;
    const int nkeys = atoi(argv[a++]);
    for (int i = 0; i < nkeys; ++i) {
        const unsigned long long u = strtoull(argv[a++], nullptr, 16);
        const unsigned long long k = ord_key(dbl(u));
        const double back = ord_unkey(k);
        unsigned long long ub; memcpy(&ub, &back, 8);
        std::printf("%%016llx %%016llx %%016llx\n", k, ub, ord_bits_of_key(ord_key_of_bits(u)));
    }
    // (j, g) of every (m, p): p as 16 hex digits
    const int nm = atoi(argv[a++]);
    const int m0 = a; a += nm;
    const int np = atoi(argv[a++]);
    for (int i = 0; i < nm; ++i)
        for (int q = 0; q < np; ++q) {
            const OrdRank r = ord_rank(dbl(strtoull(argv[a + q], nullptr, 16)), atoll(argv[m0 + i]));
            unsigned long long gb; memcpy(&gb, &r.g, 8);
            std::printf("%%lld %%016llx\n", r.j, gb);
        }
    a += np;
    // value of three (lo, hi, g)
    std::printf("%%.17g %%.17g %%.17g\n", ord_value(1.0, 2.0, 0.25), ord_value(-1.7976931348623157e308, 1e308, 0.25), ord_value(3.0, 3.0, 0.5));
    // the groups of `ncols` columns of nd draws under every cap: "nd ncols cap" triples
    while (a + 2 < argc) {
        const long long nd = atoll(argv[a]), ncols = atoll(argv[a + 1]), cap = atoll(argv[a + 2]);
        a += 3;
        const long long gc = ord_group_cols(nd, ncols, cap);
        std::printf("%%lld:", gc);
        for (const OrdGroup& g : ord_groups(ncols, gc)) std::printf(" %%lld+%%lld", g.c0, g.n);
        std::printf("\n");
    }
    return 0;
}
"""

KEY_TABLE = [-np.inf, -np.finfo(float).max, -1.0, -np.finfo(float).tiny, -5e-324, -0.0, 0.0, 5e-324, np.finfo(float).tiny, 1.0,
             np.nextafter(1.0, 2.0), np.finfo(float).max, np.inf]          # ascending in the total order


def _hex(x):
    return "%016x" % int(np.float64(x).view(np.uint64))


def test_plan_header_on_the_cpu(tmp_path):
    """csrc/order_plan.hpp, compiled by g++ -Wall -Werror into a stand-alone program and once more with
    -fsanitize=address,undefined (nothing is loaded into Python): the key map and its inverse on +-0, +-subnormal, +-1, +-max,
    +-inf; strictly ascending keys over the sorted table; the digit schedule covers the 64 bits exactly once; (j, g) over the edge
    list of m and p the GPU tests use, against the Python restatement; the column groups for W * C = 1, 7, 1380 under every
    cap: whole columns, nothing dropped, nothing twice."""
    src = tmp_path / "plan_main.cpp"
    src.write_text(PLAN_MAIN % os.path.join(ROOT, "hmc.jl_amd", "csrc", "order_plan.hpp"))
    exe, san = tmp_path / "plan_main", tmp_path / "plan_main_san"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", str(src), "-o", str(exe)])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           str(src), "-o", str(san)])
    group_cases = [(nd, ncols, cap) for ncols in (1, 7, 1380) for nd in (1, 2065, 250000, 2 ** 31 - 1)
                   for cap in (0, 1, 2, 3, 26, ncols - 1, ncols, ncols + 1, 10 ** 6)]
    args = [str(len(KEY_TABLE))] + [_hex(x) for x in KEY_TABLE]
    args += [str(len(qc.M_EDGES))] + [str(m) for m in qc.M_EDGES] + [str(len(qc.P_EDGES))] + [_hex(p) for p in qc.P_EDGES]
    for t in group_cases:
        args += [str(v) for v in t]
    out = subprocess.check_output([str(exe)] + args).decode().splitlines()
    assert subprocess.check_output([str(san)] + args).decode().splitlines() == out
    assert out[0].split() == ["8", "8", "255", "32", "4096"]
    shifts = [int(s) for s in out[1].split()]
    covered = 0
    for s in shifts:
        assert covered & (255 << s) == 0
        covered |= 255 << s
    assert covered == 2 ** 64 - 1 and shifts == sorted(shifts, reverse=True) and len(shifts) == 8      # from the top, exactly once
    keys = []
    for i, x in enumerate(KEY_TABLE):
        k, back, twice = out[2 + i].split()
        assert back == _hex(x) == twice                                         # a bijection: the bits come back
        assert int(k, 16) == int(qc.key_of(np.array([x]))[0])
        keys.append(int(k, 16))
    assert all(a < b for a, b in zip(keys, keys[1:]))                           # -0.0 below +0.0 included
    at = 2 + len(KEY_TABLE)
    for m in qc.M_EDGES:
        for p in qc.P_EDGES:
            j, gb = out[at].split()
            wj, wg = qc.rank(p, m)
            assert int(j) == wj and gb == _hex(wg) and 0 <= wj <= m - 1 and 0.0 <= wg < 1.0, (m, p)
            at += 1
    assert out[at].split() == ["1.25", "1e+308", "3"]                           # the rule, the clamp (overflow), lo == hi
    at += 1
    for nd, ncols, cap in group_cases:
        head, *groups = out[at].split()
        at += 1
        gc = int(head[:-1])
        fit = (64 << 20) // (8 * nd)
        want = min(fit, cap) if cap > 0 else fit
        assert gc == min(max(want, 1), ncols), (nd, ncols, cap)
        spans = [tuple(int(v) for v in g.split("+")) for g in groups]
        assert spans[0][0] == 0 and sum(n for _, n in spans) == ncols
        assert all(a0 + an == b0 for (a0, an), (b0, _) in zip(spans, spans[1:]))   # whole columns, none dropped, none twice
        assert all(1 <= n <= gc for _, n in spans) and all(n == gc for _, n in spans[:-1])
    assert at == len(out)


def test_reference_agrees_with_numpy_quantile():
    """On seeded normal columns the reference's value is numpy's linear quantile to three roundings of lo + g (hi - lo):
    2^-51 (|lo| + |hi|); lo and hi are np.sort's neighbours."""
    rng = np.random.default_rng(7)
    for m in (2, 3, 10, 63, 64, 65, 1000, 5000):
        x = rng.standard_normal((2, 3, m)) * np.array([1.0, 10.0, 0.01])[None, :, None] + np.array([0.0, 5.0, -2.0])[None, :, None]
        ref = qc.reference(x, qc.PROBS16, False)
        want = np.quantile(x, qc.PROBS16, axis=2, method="linear").transpose(1, 2, 0)
        assert (np.abs(ref["value"] - want) <= 2.0 ** -51 * (np.abs(ref["lo"]) + np.abs(ref["hi"]))).all(), m
        s = np.sort(x, axis=2)
        for i, p in enumerate(qc.PROBS16):
            j, _ = qc.rank(p, m)
            assert np.array_equal(ref["lo"][:, :, i], s[:, :, j]) and np.array_equal(ref["hi"][:, :, i], s[:, :, min(j + 1, m - 1)])
        assert (ref["count"] == m).all() and (ref["nan"] == 0).all()


def test_reference_orders_zeros_counts_nans_and_clamps():
    x = np.array([[[0.0, -0.0, -0.0, np.nan]]])
    ref = qc.reference(x, (0.0, 1.0), False)
    assert ref["count"][0, 0] == 3 and ref["nan"][0, 0] == 1
    assert np.signbit(ref["lo"][0, 0, 0]) and not np.signbit(ref["lo"][0, 0, 1])
    ref = qc.reference(np.full((1, 1, 5), np.nan), (0.5,), True)
    assert ref["count"][0, 0] == 0 and np.isnan([ref[k][0, 0, 0] for k in qc.FIELDS]).all()
    ref = qc.reference(np.array([[[qc.CLAMP_HI, qc.CLAMP_LO]]]), (qc.CLAMP_P,), False)
    assert ref["g"][0, 0, 0] == 0.25 and ref["value"][0, 0, 0] == qc.CLAMP_HI          # inf without the clamp
    ref = qc.reference(np.array([[[-np.inf, 1.0, 2.0]]]), (0.25, 0.0), False)
    assert np.isnan(ref["value"][0, 0, 0]) and ref["value"][0, 0, 1] == -np.inf
    assert np.array_equal(qc.round5(np.array([-1e-9])).view(np.int64), np.array([-0.0]).view(np.int64))     # a cell keeps the sign


def _hand_made(seed, K=3, n=300):
    """Draws in the reference's Julia shapes: means, variances, states (n, K), A (n, K, K) with A[d, i, j]."""
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((n, K)) + 3.0 * np.arange(K)
    variances = 0.05 + rng.gamma(2.0, 0.8, size=(n, K))
    states = rng.dirichlet(np.ones(K), size=n)
    A = rng.dirichlet(np.ones(K) * 2.0, size=(n, K))
    return means, variances, states, A


def test_calcquantiles_file_route_and_writer(tmp_path):
    """Per-draw files written by hmc.saveresults from hand-made draws (K = 3, n = 300, two dates) through hmc.calcquantiles
    (numpy, no GPU) against quantile_cases.reference on the same draws, rounded as the cells are: bit for bit; then the
    writer's text."""
    dates = [dt.date(1980, 1, 1), dt.date(1985, 1, 1)]
    draws = [_hand_made(51 + i) for i in range(2)]
    for d, (means, variances, states, A) in zip(dates, draws):
        n, K = means.shape
        ds = [dt.date(1960 + i // 12, i % 12 + 1, 1) for i in range(11)] + [d]
        opt = hmc.estopt(np.zeros(12), ds, sampleRange=range(1, 13), endIndex=12, horizons=(12,), D=K, burnin=1, Nrun=n)
        hmc.saveresults(hmc.Samples(means, variances, states[:, None, :], A, np.zeros((n, 2)), [d] * n), opt, str(tmp_path), native=False)
    abi = {"mu": np.stack([m.T for m, _, _, _ in draws]), "sig2": np.stack([v.T for _, v, _, _ in draws]),
           "A": np.stack([np.transpose(a, (2, 1, 0)) for _, _, _, a in draws])}
    probs = (0.05, 0.5, 0.95, 0.0, 1.0)
    for var in ("mu", "sig2", "A"):
        got_dates, q = hmc.calcquantiles(str(tmp_path), dates, var, probs)
        assert got_dates == [str(x) for x in dates] and q.probs == probs and q.var == var
        assert q.columns == (["trans_%d_%d" % (i, j) for j in (1, 2, 3) for i in (1, 2, 3)] if var == "A" else ["state_1", "state_2", "state_3"])
        ref = qc.reference(abi[var], probs, True)
        assert q.value.shape == (2, len(q.columns), 5)
        qc.check({k: getattr(q, k) for k in qc.FIELDS + ("count", "nan")}, ref, var)
        assert np.array_equal(qc.bits(q.value), qc.bits(ref["value"]))
    _, mu = hmc.calcquantiles(str(tmp_path), dates, "mu")
    assert mu.probs == (0.05, 0.5, 0.95) and (np.abs(mu.value[:, :, 1] - 3.0 * np.arange(3)) < 0.3).all()      # the medians
    one = mu.rows([1])
    assert one.value.shape == (1, 3, 3) and np.array_equal(one.lo, mu.lo[1:]) and np.array_equal(one.count, mu.count[1:])
    with pytest.raises(FileNotFoundError):
        hmc.calcquantiles(str(tmp_path), [dt.date(1990, 1, 1)])
    with pytest.raises(ValueError, match="probs"):
        hmc.calcquantiles(str(tmp_path), dates, "mu", (0.5, 1.5))
    with pytest.raises(ValueError, match="var must be"):
        hmc.calcquantiles("unused", [], "x")
    path = hmc.write_chain_quantiles(str(tmp_path / "chain_quantiles.csv"), [str(x) for x in dates], mu)
    header, rows = hmc._read_csv(path)
    assert header == ["date", "column", "prob", "value", "lo", "hi", "g", "count", "nan"] and len(rows) == 2 * 3 * 3
    r = rows[(1 * 3 + 2) * 3 + 1]
    assert r[:3] == ["1985-01-01", "state_3", "0.5"] and r[3] == hmc._fmt(mu.value[1, 2, 1]) and r[4] == hmc._fmt(mu.lo[1, 2, 1])
    assert r[5] == hmc._fmt(mu.hi[1, 2, 1]) and r[6] == hmc._fmt(mu.g[1, 2, 1]) and r[7:] == ["300", "0"]


def test_batchresult_quantiles_is_none_unless_asked_for():
    res = hmc.BatchResult([], {"summary": np.zeros((0, 1)), "status": np.zeros(0, dtype=np.int32)}, False)
    assert res.quantiles is None
    with pytest.raises(ValueError, match="no quantiles"):
        hmc.calcquantiles("unused", ["1980-01-01"], "mu", result=res)
    empty = {k: np.zeros((0, 3, 3)) for k in qc.FIELDS}
    empty.update({"count": np.zeros((0, 3), dtype=np.int64), "nan": np.zeros((0, 3), dtype=np.int64)})
    res.quantiles = {"mu": hmc.ChainQuantiles("mu", ["state_1", "state_2", "state_3"], (0.05, 0.5, 0.95), empty)}
    with pytest.raises(ValueError, match="no quantiles of sig2"):
        hmc.calcquantiles("unused", [], "sig2", result=res)
    with pytest.raises(ValueError, match="other probabilities"):
        hmc.calcquantiles("unused", [], "mu", (0.5,), result=res)
    assert hmc.calcquantiles("unused", [], "mu", result=res)[1].value.shape == (0, 3, 3)
    with pytest.raises(ValueError, match="quantile_vars"):
        hmc.estimatewindows(np.zeros(12), [dt.date(1960, 1, 1)] * 12, [12], quantile_vars=("x",))
