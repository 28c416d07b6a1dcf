"""Chain densities and running means of the draws (hmcg_chain_density; plots/mcplots.jl, plots/timeseriesplots.jl): the parts
that need no GPU -- the struct and the argument rules of the built library (checked before device init), csrc/density_plan.hpp
run by a g++-compiled program (also under AddressSanitizer and UBSan), the reference's histogram against np.histogram,
hmc.chainquantiles against a sort, hmc.chaindensity against the direct Gaussian sum, the file route of hmc.calcchain and the
writers."""
import ctypes as C
import datetime as dt
import os
import subprocess

import numpy as np
import pytest

import hmc_jl_amd
from hmc_jl_amd import _lib, hmc

import density_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSITY = _lib.Density                # the whole module is about this feature: without the binding none of it runs


def test_ctypes_struct_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%%zu %%d %%d %%d %%d %%zu %%zu %%zu %%d", '
                   'sizeof(hmcg_density), HMCG_DENS_ROUND5, HMCG_DENS_MAXBINS, HMCG_DENS_MAXTRACE, HMCG_MAXH, offsetof(hmcg_density, cuts), '
                   'offsetof(hmcg_density, trace_len), offsetof(hmcg_density, trace_stride), HMCG_VERSION);return 0;}\n'
                   % os.path.join(ROOT, "include", "hmcg.h"))
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    D = DENSITY
    assert got[:8] == [C.sizeof(D), _lib.DENS_ROUND5, _lib.DENS_MAXBINS, _lib.DENS_MAXTRACE, _lib.HMCG_MAXH, D.cuts.offset,
                       D.trace_len.offset, D.trace_stride.offset]
    assert C.sizeof(D) == 120 and _lib.DENS_MAXBINS == 512 and _lib.DENS_MAXTRACE == 65536
    assert got[8] == 109 == hmc_jl_amd.load().hmcg_version()              # additions only: the version stays
    assert {"hmcg_chain_density", "hmcg_chain_density_device"} <= set(_lib.EXPORTS)
    assert _lib.DENS_FIELDS == ("counts", "below", "above", "nan", "range", "mean", "variance", "trace")


MISUSE = [
    (dict(struct_size=7), {}, b"struct_size"),
    (dict(W=0), {}, b"at least one window"),
    (dict(C=0), {}, b"C = 0"),
    (dict(C=65), {}, b"C = 65"),
    (dict(B=0), {}, b"B = 0"),
    (dict(B=513), {}, b"B = 513"),
    (dict(nd=0), {}, b"at least one draw"),
    (dict(nd=2 ** 53 + 1, nd_ld=2 ** 53 + 1), {}, b"exceeds 2^53"),
    (dict(nd_ld=3), {}, b"nd_ld"),
    (dict(n_cuts=0), {}, b"n_cuts = 0"),
    (dict(n_cuts=9), {}, b"n_cuts = 9"),
    (dict(cut0=0), {}, b"cut 0 outside"),
    (dict(cut1=5), {}, b"cut 5 outside"),
    (dict(cut0=4), {}, b"not strictly ascending"),
    (dict(cut1=2), {}, b"not strictly ascending"),
    (dict(trace_len=-1), {}, b"trace_len = -1"),
    (dict(trace_len=65537), {}, b"trace_len = 65537"),
    (dict(trace_stride=0), {}, b"trace_stride = 0"),
    (dict(trace_len=2, trace_stride=3), {}, b"trace_len * trace_stride"),
    (dict(W=2 ** 31 - 1, nd=2 ** 40, nd_ld=2 ** 40), {}, b"W * pieces * column groups exceeds one launch"),
    (dict(W=2 ** 29, C=64), {}, b"W * C exceeds one launch"),
    ({}, dict(x=False), b"required"),
    ({}, dict(range=False), b"required"),
    ({}, dict(counts=False), b"required"),
    ({}, dict(stats=False), b"required"),
    ({}, dict(trace=False), b"trace is NULL"),
]
HOST_MISUSE = [(np.nan, 1.0), (0.0, np.inf), (1.0, 0.5), (-np.inf, 0.0)]


@pytest.mark.parametrize("entry", ["hmcg_chain_density", "hmcg_chain_density_device"])
def test_misuse_is_refused_before_device_init(entry):
    """Every rule returns HMCG_E_BADARG with its text from the built library; the data pointers are never followed (the device
    entry is handed host addresses here) and no GPU is needed: the check precedes get_context.  The host entry also reads
    lo_hi, which is host memory there."""
    lib = hmc_jl_amd.load()
    buf = np.zeros(64)
    ok = C.c_void_p(buf.ctypes.data)
    device = entry.endswith("device")

    def call(p, a):
        args = [C.byref(p), a["x"], a["lo_hi"], a["range"], a["counts"], a["stats"], a["trace"]] + ([None] if device else []) + [None]
        return getattr(lib, entry)(*args)
    names = ("x", "lo_hi", "range", "counts", "stats", "trace")
    for fields, ptrs, text in MISUSE:
        p = _lib.make_density(1, 3, 4, 4, (3, 4), 8, (1, 2))
        for k, v in fields.items():
            if k.startswith("cut"):
                p.cuts[int(k[3:])] = v
            else:
                setattr(p, k, v)
        a = {n: (ok if ptrs.get(n, True) else None) for n in names}
        rc = call(p, a)
        assert rc == -1 and text in lib.hmcg_last_error(), (fields, ptrs, rc, lib.hmcg_last_error())
    if not device:
        for lo, hi in HOST_MISUSE:
            lh = np.zeros((1, 3, 2))
            lh[0, 1] = lo, hi
            a = {n: ok for n in names}
            a["lo_hi"] = C.c_void_p(lh.ctypes.data)
            rc = call(_lib.make_density(1, 3, 4, 4, (3, 4), 8, (1, 2)), a)
            assert rc == -1 and b"finite with hi >= lo" in lib.hmcg_last_error(), (lo, hi, rc, lib.hmcg_last_error())
    with pytest.raises(ValueError, match="at most 8 cuts"):
        _lib.make_density(1, 3, 40, 40, tuple(range(1, 10)))


# Two rules broken at once: the rule the entry names first, with its whole text.  The order is this feature's own (B stands
# between C and nd); the texts of the rules it shares with the other draw statistics come from csrc/stat_plan.hpp.
DOUBLY_WRONG = [
    (dict(struct_size=7, W=0), b"hmcg_density.struct_size 7 != %d" % C.sizeof(_lib.Density)),
    (dict(W=0, nd_ld=3), b"W = 0: at least one window"),
    (dict(C=0, nd=0), b"C = 0 columns outside 1..64"),
    (dict(B=0, nd=0), b"B = 0 bins outside 1..512"),
    (dict(nd=0, nd_ld=-1), b"nd = 0: at least one draw"),
    (dict(nd=2 ** 53 + 1, nd_ld=4), b"nd = 9007199254740993 exceeds 2^53, the largest exact divisor"),
    (dict(nd_ld=3, n_cuts=0), b"nd_ld = 3 < nd = 4"),
    (dict(W=2 ** 29, C=64, trace_len=0), b"W * C exceeds one launch (2^31 - 1 blocks)"),
]


@pytest.mark.parametrize("fields, message", DOUBLY_WRONG)
@pytest.mark.parametrize("entry", ["hmcg_chain_density", "hmcg_chain_density_device"])
def test_first_rule_named_for_a_doubly_wrong_call(entry, fields, message):
    lib = hmc_jl_amd.load()
    buf = np.zeros(64)
    ok = C.c_void_p(buf.ctypes.data)
    p = _lib.make_density(1, 3, 4, 4, (3, 4), 8, (1, 2))
    for k, v in fields.items():
        setattr(p, k, v)
    trace = None if fields.get("trace_len") == 0 else ok       # ... and with trace_len = 0 the missing x, were it reached
    rc = getattr(lib, entry)(C.byref(p), None if trace is None else ok, None, ok, ok, ok, trace,
                             *(([None] if entry.endswith("device") else []) + [None]))
    assert rc == -1 and lib.hmcg_last_error() == message


PLAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "%s"
// argv: nd cut...   prints: pieces, then one line per piece "d0 n segment piece_of(d0) piece_of(d0 + n - 1)", then piece_of(nd)
int main(int argc, char** argv)
{
    using namespace hmcg_host;
    if (argc == 1) {                     // constants and the column groups of every (C, B)
        std::printf("%%lld %%d %%d\n", PRED_SLAB, DENS_SLOTS, DENS_LDS_WORDS);
        int bad = 0;
        for (int C = 1; C <= HMCG_MAXK * HMCG_MAXK; ++C)
            for (int B = 1; B <= HMCG_DENS_MAXBINS; ++B) {
                const int g = dens_group_cols(C, B), n = dens_groups(C, B);
                if (g < 1 || g > C || g * (B + DENS_SLOTS) > DENS_LDS_WORDS || n * g < C || (n - 1) * g >= C) ++bad;
            }
        std::printf("%%d %%d %%d %%d %%d\n", bad, dens_group_cols(3, 64), dens_groups(3, 64), dens_group_cols(64, 512), dens_groups(64, 512));
        return 0;
    }
    const long long nd = std::atoll(argv[1]);
    int64_t cuts[HMCG_MAXH] = {};
    const int n_cuts = argc - 2;
    for (int j = 0; j < n_cuts; ++j) cuts[j] = std::atoll(argv[2 + j]);
    const long long np = dens_pieces(nd, cuts, n_cuts);
    std::printf("%%lld\n", np);
    for (long long q = 0; q < np; ++q) {
        const DensPiece p = dens_piece(q, nd, cuts, n_cuts);
        std::printf("%%lld %%lld %%d %%lld %%lld\n", p.d0, p.n, p.segment, dens_piece_of(p.d0, nd, cuts, n_cuts),
                    dens_piece_of(p.d0 + p.n - 1, nd, cuts, n_cuts));
    }
    std::printf("%%lld\n", dens_piece_of(nd, nd, cuts, n_cuts));
    return 0;
}
"""


def _plan_cut_sets(nd):
    """Cuts at 1, at a slab boundary, inside a slab, two in one slab and at nd, as far as nd has room for them."""
    S = dc.SLAB
    sets = [(nd,), (1,), tuple(sorted({1, nd}))]
    if nd >= S:
        sets.append(tuple(sorted({S, nd})))
    if nd >= 3:
        sets.append((nd // 2,))
        sets.append(tuple(sorted({nd // 3, 2 * nd // 3 + 1, nd})))
    if nd > S + 2:
        sets.append((S + 1, S + 2))
        sets.append(tuple(sorted({1, 5, S, S + 1, 2 * S, nd - 1, nd} & set(range(1, nd + 1)))))
    sets.append(dc.cut_set(4, nd))
    return [s for s in dict.fromkeys(sets) if all(1 <= c <= nd for c in s)]


def _check_plan(exe, nd, cuts):
    S = dc.SLAB
    out = subprocess.check_output([str(exe), str(nd)] + [str(c) for c in cuts]).decode().split("\n")
    npieces = int(out[0])
    pieces = [tuple(int(v) for v in line.split()) for line in out[1:1 + npieces]]
    assert int(out[1 + npieces]) == npieces
    assert npieces <= (nd + S - 1) // S + len(cuts)
    bounds = sorted(set(range(0, nd, S)) | {c for c in cuts if c < nd})
    assert [p[0] for p in pieces] == bounds, (nd, cuts)                    # exactly the union of slab starts and cuts
    pos = 0
    for q, (d0, n, seg, q_first, q_last) in enumerate(pieces):
        assert d0 == pos and 1 <= n <= S, (nd, cuts, q)                    # in order, no gap, no overlap
        assert d0 // S == (d0 + n - 1) // S, (nd, cuts, q, "crosses a slab boundary")
        assert not any(d0 < c < d0 + n for c in cuts), (nd, cuts, q, "crosses a cut")
        assert seg == sum(1 for c in cuts if c <= d0), (nd, cuts, q)
        assert q_first == q == q_last
        pos = d0 + n
    assert pos == nd


def test_plan_header_pieces_and_column_groups(tmp_path):
    """csrc/density_plan.hpp, compiled by g++ -Wall -Werror into a stand-alone program and once more with
    -fsanitize=address,undefined: the pieces tile [0, nd) in order, none crosses a slab boundary or a cut, their segments count
    the cuts at or before them, the inverse map agrees, and the column groups of every (C, B) fit the LDS budget and cover C."""
    src = tmp_path / "plan_main.cpp"
    src.write_text(PLAN_MAIN % os.path.join(ROOT, "hmc.jl_amd", "csrc", "density_plan.hpp"))
    exe, san = tmp_path / "plan_main", tmp_path / "plan_main_san"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", str(src), "-o", str(exe)])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           str(src), "-o", str(san)])
    head = subprocess.check_output([str(exe)]).decode().splitlines()
    assert head[0].split() == ["1024", "3", "8192"] and _lib.PRED_SLAB == 1024 == dc.SLAB
    assert head[1].split() == ["0", "3", "1", "15", "5"]                  # C = 64, B = 512: 15 columns a block, 5 groups
    assert subprocess.check_output([str(san)]).decode().splitlines() == head
    n_sets = 0
    for nd in dc.ND:
        for cuts in _plan_cut_sets(nd):
            _check_plan(exe, nd, cuts)
            n_sets += 1
    assert n_sets >= 40
    for nd, cuts in ((2065, (1, 5, 1024, 1025, 2048, 2064, 2065)), (1, (1,)), (250000, (100000, 150000, 200000, 250000))):
        _check_plan(san, nd, cuts)


def test_reference_histogram_against_numpy():
    """On clean data the bin rule is np.histogram's: equal-width bins, the last one closed.  The draws keep a tenth of a bin
    away from every inner edge (np.histogram places by searching its own edge array, which may differ from the rule in the
    last ulp there), the two ends of the range are among them, and the comparison is exact."""
    rng = np.random.default_rng(5)
    lo, hi = -2.0, 6.0
    for B in (1, 2, 7, 64, 512):
        n = 3000
        idx = np.clip(np.rint(rng.normal(B / 2.0, B / 6.0 + 0.5, size=n)), 0, B - 1)
        v = lo + (idx + rng.uniform(0.1, 0.9, size=n)) * ((hi - lo) / B)
        v[17], v[1500] = lo, hi                                          # one end in each prefix
        x = v[None, None, :]
        ref = dc.reference(x, (1000, n), B, None, (0, 1), False)
        assert tuple(ref["range"][0, 0]) == (lo, hi)
        for j, cut in enumerate((1000, n)):
            want, _ = np.histogram(v[:cut], bins=B, range=(lo, hi))
            assert np.array_equal(ref["counts"][0, 0, j], want), (B, cut)
            assert ref["below"][0, 0, j] == ref["above"][0, 0, j] == ref["nan"][0, 0, j] == 0
    # every special slot, by hand
    v = np.array([np.nan, -np.inf, np.inf, -1.0, 0.0, -0.0, 0.25, 0.5, 1.0, 1.5])
    assert list(dc.histogram(v, 0.0, 1.0, 4)) == [-3, -1, -2, -1, 0, 0, 1, 2, 3, -2]
    assert list(dc.histogram(v, 0.5, 0.5, 4)) == [-3, -1, -2, -1, -1, -1, -1, 0, -2, -2]
    assert list(dc.histogram(v, np.nan, np.nan, 4)) == [-3] + [-1] * 9
    assert list(dc.round5(np.array([1.000004, 1.000006, np.inf, 1e308, -0.0]))) == [1.0, 1.00001, np.inf, 1e308, 0.0]


def _density_of(x, cuts, bins, trace=(0, 1), lo_hi=None):
    """A ChainDensity from the reference on x (W, C, nd), no rounding."""
    ref = dc.reference(x, cuts, bins, lo_hi, trace, False)
    parts = {k: np.asarray(ref[k], dtype=np.float64 if k in ("mean", "variance", "trace", "range") else np.int64) for k in _lib.DENS_FIELDS}
    return hmc.ChainDensity("mu", ["state_%d" % (i + 1) for i in range(x.shape[1])], ref["cuts"], trace[1], parts)


def test_chainquantiles_against_a_sort():
    rng = np.random.default_rng(6)
    x = dc.make_case(3, 2, 9, 700, 0, 32)
    cuts, B = (100, 700), 32
    for lo_hi in (None, dc.given_range(1, dc.reference(x, cuts, B, None, (0, 1), False), 2, 9)):
        d = _density_of(x, cuts, B, lo_hi=lo_hi)
        qs = (0.0, 0.025, 0.25, 0.5, 0.975, 1.0, float(rng.random()))
        got = hmc.chainquantiles(d, qs)
        for w in range(2):
            for c in range(9):
                lo, hi = d.range[w, c]
                for j, cut in enumerate(cuts):
                    v = x[w, c, :cut]
                    v = np.sort(v[~np.isnan(v)])
                    for i, q in enumerate(qs):
                        if v.size == 0:
                            assert got["bin"][w, c, j, i] == -1 and np.isnan(got["lo"][w, c, j, i])
                            continue
                        k = min(max(int(np.ceil(q * v.size)), 1), v.size)
                        slot = int(dc.histogram(v[k - 1:k], lo, hi, B)[0])
                        want = {-1: -1, -2: B}.get(slot, slot)
                        assert got["bin"][w, c, j, i] == want, (w, c, j, q)
                        if 0 <= want < B and hi > lo:
                            # the edges bracket the order statistic up to the rounding of the edge itself
                            eps = 4 * np.finfo(float).eps * max(abs(lo), abs(hi))
                            assert got["lo"][w, c, j, i] - eps <= v[k - 1] <= got["hi"][w, c, j, i] + eps


def test_chaindensity_against_the_direct_gaussian_sum():
    """Data lying on bin centres: binning loses nothing, so the estimate from the counts is the kernel sum over the data itself
    with the same bandwidth; and that bandwidth is Silverman's rule."""
    rng = np.random.default_rng(7)
    B, n = 40, 5000
    lo, hi = -2.0, 6.0
    width = (hi - lo) / B
    idx = np.clip(np.rint(rng.normal(20, 5, size=n)), 0, B - 1).astype(int)
    data = lo + (idx + 0.5) * width
    x = data[None, None, :]
    d = _density_of(x, (n // 2, n), B, lo_hi=np.array([[[lo, hi]]]))
    assert d.counts.sum() == n + n // 2
    for pts in (None, np.linspace(-3.0, 7.0, 57)):
        got = hmc.chaindensity(d, pts)
        for j, cut in enumerate((n // 2, n)):
            h = got["bandwidth"][0, 0, j]
            v = data[:cut]
            q25, q75 = np.sort(v)[int(np.ceil(0.25 * cut)) - 1], np.sort(v)[int(np.ceil(0.75 * cut)) - 1]
            want_h = 0.9 * min(v.std(ddof=1), (q75 - q25) / 1.34) * cut ** -0.2
            assert abs(h - want_h) <= 1e-12 * want_h
            px = got["x"][0, 0]
            direct = np.exp(-0.5 * ((px[:, None] - v[None, :]) / h) ** 2).sum(axis=1) / (cut * h * np.sqrt(2 * np.pi))
            assert np.abs(got["density"][0, 0, j] - direct).max() <= 1e-12 * direct.max()
        if pts is None:
            assert np.allclose(got["x"][0, 0], lo + (np.arange(B) + 0.5) * width, rtol=0, atol=1e-12)
            assert abs(got["density"][0, 0, 1].sum() * width - 1.0) < 1e-3           # a density
    assert (hmc.chaindensity(d, None, bandwidth=0.5)["bandwidth"] == 0.5).all()


def _hand_made(seed, K=3, n=300):
    """Draws in the reference's Julia shapes: means, variances, states (n, K), A (n, K, K) with A[d, i, j]."""
    rng = np.random.default_rng(seed)
    means = np.sort(rng.normal(3.0, 2.5, size=(n, K)), axis=1)
    variances = 0.05 + rng.gamma(2.0, 0.8, size=(n, K))
    states = rng.dirichlet(np.ones(K), size=n)
    A = rng.dirichlet(np.ones(K) * 2.0, size=(n, K))
    return means, variances, states, A


def test_calcchain_file_route_and_writers(tmp_path):
    """Per-draw files written by hmc.saveresults from hand-made draws (K = 3, n = 300, two dates) through hmc.calcchain (numpy,
    no GPU) against density_cases.reference on the same draws, rounded as the cells are; then the two writers' text."""
    dates = [dt.date(1980, 1, 1), dt.date(1985, 1, 1)]
    draws = [_hand_made(41 + i) for i in range(2)]
    for d, (means, variances, states, A) in zip(dates, draws):
        n, K = means.shape
        ds = [dt.date(1960 + i // 12, i % 12 + 1, 1) for i in range(11)] + [d]
        opt = hmc.estopt(np.zeros(12), ds, sampleRange=range(1, 13), endIndex=12, horizons=(12,), D=K, burnin=1, Nrun=n)
        hmc.saveresults(hmc.Samples(means, variances, states[:, None, :], A, np.zeros((n, 2)), [d] * n), opt, str(tmp_path), native=False)
    cuts, B, trace = (100, 250, 300), 16, (42, 7)
    abi = {"mu": np.stack([m.T for m, _, _, _ in draws]), "sig2": np.stack([v.T for _, v, _, _ in draws]),
           "A": np.stack([np.transpose(a, (2, 1, 0)) for _, _, _, a in draws])}
    for var in ("mu", "sig2", "A"):
        got_dates, d = hmc.calcchain(str(tmp_path), dates, var, cuts, B, None, trace)
        assert got_dates == [str(x) for x in dates] and d.cuts == cuts and d.bins == B and d.trace_stride == 7
        assert d.columns == (["trans_%d_%d" % (i, j) for j in (1, 2, 3) for i in (1, 2, 3)] if var == "A" else ["state_1", "state_2", "state_3"])
        ref = dc.reference(abi[var], cuts, B, None, trace, True)
        dc.check({k: getattr(d, k) for k in _lib.DENS_FIELDS}, ref, "files %s" % var)
    _, whole = hmc.calcchain(str(tmp_path), dates[:1], "mu", bins=B)
    _, explicit = hmc.calcchain(str(tmp_path), dates[:1], "mu", (300,), B)
    assert whole.cuts == (300,) and np.array_equal(whole.counts, explicit.counts) and (whole.counts.sum(axis=3) == 300).all()
    lh = np.tile(np.array([0.0, 5.0]), (2, 3, 1))
    _, given = hmc.calcchain(str(tmp_path), dates, "mu", cuts, B, lh, trace)
    dc.check({k: getattr(given, k) for k in _lib.DENS_FIELDS}, dc.reference(abi["mu"], cuts, B, lh, trace, True), "files, given range")
    assert (given.below + given.above).sum() > 0
    with pytest.raises(FileNotFoundError):
        hmc.calcchain(str(tmp_path), [dt.date(1990, 1, 1)])
    with pytest.raises(ValueError, match="beyond"):
        hmc.calcchain(str(tmp_path), dates, "mu", (301,))
    # the writers
    _, d = hmc.calcchain(str(tmp_path), dates, "mu", cuts, B, None, trace)
    path = hmc.write_chain_density(str(tmp_path / "chain_density.csv"), [str(x) for x in dates], d)
    header, rows = hmc._read_csv(path)
    assert header == ["date", "column", "cut", "bin_lo", "bin_hi", "count", "density"] and len(rows) == 2 * 3 * 3 * B
    kde = hmc.chaindensity(d)["density"]
    r = rows[((1 * 3 + 2) * 3 + 1) * B + 5]                               # date 1, column 2, cut 1, bin 5
    lo, hi = d.range[1, 2]
    assert r[:3] == ["1985-01-01", "state_3", "250"] and int(r[5]) == d.counts[1, 2, 1, 5]
    assert r[3] == hmc._fmt(lo + 5 * ((hi - lo) / B)) and r[4] == hmc._fmt(lo + 6 * ((hi - lo) / B)) and r[6] == hmc._fmt(kde[1, 2, 1, 5])
    assert sum(int(x[5]) for x in rows if x[0] == "1980-01-01" and x[1] == "state_1" and x[2] == "300") == 300
    path = hmc.write_chain_trace(str(tmp_path / "chain_trace.csv"), [str(x) for x in dates], d)
    header, rows = hmc._read_csv(path)
    assert header == ["date", "column", "draws", "mean"] and len(rows) == 2 * 3 * 42
    assert rows[42 + 3] == ["1980-01-01", "state_2", "28", hmc._fmt(d.trace[0, 1, 3])]


def test_batchresult_density_is_none_unless_asked_for():
    res = hmc.BatchResult([], {"summary": np.zeros((0, 1)), "status": np.zeros(0, dtype=np.int32)}, False)
    assert res.density is None
    with pytest.raises(ValueError, match="no chain density"):
        hmc.calcchain("unused", ["1980-01-01"], "mu", result=res)
    empty = {"counts": np.zeros((0, 3, 1, 8), dtype=np.int64), "range": np.zeros((0, 3, 2)), "trace": np.zeros((0, 3, 0))}
    empty.update({k: np.zeros((0, 3, 1)) for k in ("below", "above", "nan", "mean", "variance")})
    res.density = {"mu": hmc.ChainDensity("mu", ["state_1", "state_2", "state_3"], (50,), 1, empty)}
    with pytest.raises(ValueError, match="no chain density of sig2"):
        hmc.calcchain("unused", [], "sig2", result=res)
    with pytest.raises(ValueError, match="other cuts, bins or trace"):
        hmc.calcchain("unused", [], "mu", (50,), 16, result=res)
    assert hmc.calcchain("unused", [], "mu", (50,), 8, result=res)[1].counts.shape == (0, 3, 1, 8)
    with pytest.raises(ValueError, match="var must be"):
        hmc.calcchain("unused", [], "x")
