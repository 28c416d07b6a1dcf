"""Autocorrelation, effective sample size and split-R-hat of the draws (hmcg_chain_autocorr): the parts that need no GPU -- the
struct and the argument rules of the built library (checked before device init), csrc/autocorr_plan.hpp run by a g++-compiled
program (also under AddressSanitizer and UBSan) against a Python restatement, the reference's rules on AR(1) chains whose
integrated autocorrelation time is known, the split-R-hat on white noise and on a shifted chain, the file route of hmc.calcess
and the writer."""
import ctypes as C
import datetime as dt
import os
import subprocess

import numpy as np
import pytest

import hmc_jl_amd
from hmc_jl_amd import _lib, hmc

import autocorr_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUTOCORR = _lib.Autocorr              # the whole module is about this feature: without the binding none of it runs


def test_ctypes_struct_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){printf("%%zu %%d %%d %%d %%zu %%zu %%zu %%d", '
                   'sizeof(hmcg_autocorr), HMCG_ACF_ROUND5, HMCG_ACF_MAXLAG, HMCG_ACF_STRIDE, offsetof(hmcg_autocorr, nd), '
                   'offsetof(hmcg_autocorr, L), offsetof(hmcg_autocorr, flags), HMCG_VERSION);return 0;}\n'
                   % os.path.join(ROOT, "include", "hmcg.h"))
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    A = AUTOCORR
    assert got[:7] == [C.sizeof(A), _lib.ACF_ROUND5, _lib.ACF_MAXLAG, _lib.ACF_STRIDE, A.nd.offset, A.L.offset, A.flags.offset]
    assert C.sizeof(A) == 40 and _lib.ACF_MAXLAG == 1024 == ac.SLAB and _lib.ACF_STRIDE == 8 == len(_lib.ACF_FIELDS)
    assert got[7] == 109 == hmc_jl_amd.load().hmcg_version()              # additions only: the version stays
    assert {"hmcg_chain_autocorr", "hmcg_chain_autocorr_device"} <= set(_lib.EXPORTS)
    assert _lib.ACF_FIELDS == ac.FIELDS == ("mean", "variance", "tau", "ess", "mcse", "pairs", "truncated", "rhat")


MISUSE = [
    (dict(struct_size=7), {}, b"struct_size"),
    (dict(W=0), {}, b"at least one window"),
    (dict(C=0), {}, b"C = 0"),
    (dict(C=65), {}, b"C = 65"),
    (dict(nd=0, L=0), {}, b"at least one draw"),
    (dict(nd=2 ** 53 + 1, nd_ld=2 ** 53 + 1), {}, b"exceeds 2^53"),
    (dict(nd_ld=39), {}, b"nd_ld"),
    (dict(L=-1), {}, b"L = -1"),
    (dict(L=1025, nd=5000, nd_ld=5000), {}, b"L = 1025"),
    (dict(L=40), {}, b"L = 40 exceeds nd - 1 = 39"),
    (dict(nd=1, nd_ld=1, L=1), {}, b"exceeds nd - 1 = 0"),
    (dict(W=2 ** 29, C=64), {}, b"W * C exceeds one launch"),
    ({}, dict(x=False), b"required"),
    ({}, dict(acov=False), b"required"),
    ({}, dict(diag=False), b"required"),
]


@pytest.mark.parametrize("entry", ["hmcg_chain_autocorr", "hmcg_chain_autocorr_device"])
def test_misuse_is_refused_before_device_init(entry):
    """Every rule returns HMCG_E_BADARG with its text from the built library; the data pointers are never followed (the device
    entry is handed host addresses here) and no GPU is needed: the check precedes get_context."""
    lib = hmc_jl_amd.load()
    buf = np.zeros(64)
    ok = C.c_void_p(buf.ctypes.data)
    device = entry.endswith("device")
    names = ("x", "acov", "diag")
    for fields, ptrs, text in MISUSE:
        p = _lib.make_autocorr(1, 3, 40, 40, 7)
        for k, v in fields.items():
            setattr(p, k, v)
        a = [ok if ptrs.get(n, True) else None for n in names]
        rc = getattr(lib, entry)(C.byref(p), *(a + ([None] if device else []) + [None]))
        assert rc == -1 and text in lib.hmcg_last_error(), (fields, ptrs, rc, lib.hmcg_last_error())
    rc = getattr(lib, entry)(None, ok, ok, ok, *(([None] if device else []) + [None]))
    assert rc == -1 and b"hmcg_autocorr is NULL" in lib.hmcg_last_error()
    with pytest.raises(_lib.HmcgError, match="exceeds nd - 1"):
        _lib.chain_autocorr(np.zeros((1, 3, 4)), lags=4)


# Two rules broken at once: the rule the entry names first, with its whole text.  The order is this feature's own; the texts of
# the rules it shares with the other draw statistics come from csrc/stat_plan.hpp.
DOUBLY_WRONG = [
    (dict(struct_size=7, W=0), b"hmcg_autocorr.struct_size 7 != %d" % C.sizeof(_lib.Autocorr)),
    (dict(W=0, nd_ld=39), b"W = 0: at least one window"),
    (dict(C=65, nd=0), b"C = 65 columns outside 1..64"),
    (dict(nd=0, nd_ld=-1), b"nd = 0: at least one draw"),
    (dict(nd=2 ** 53 + 1, nd_ld=4), b"nd = 9007199254740993 exceeds 2^53, the largest exact divisor"),
    (dict(nd_ld=39, L=-1), b"nd_ld = 39 < nd = 40"),
    (dict(L=40, W=2 ** 29, C=64), b"L = 40 exceeds nd - 1 = 39"),
]


@pytest.mark.parametrize("fields, message", DOUBLY_WRONG)
@pytest.mark.parametrize("entry", ["hmcg_chain_autocorr", "hmcg_chain_autocorr_device"])
def test_first_rule_named_for_a_doubly_wrong_call(entry, fields, message):
    lib = hmc_jl_amd.load()
    buf = np.zeros(64)
    ok = C.c_void_p(buf.ctypes.data)
    p = _lib.make_autocorr(1, 3, 40, 40, 7)
    for k, v in fields.items():
        setattr(p, k, v)
    rc = getattr(lib, entry)(C.byref(p), ok, ok, ok, *(([None] if entry.endswith("device") else []) + [None]))
    assert rc == -1 and lib.hmcg_last_error() == message


PLAN_MAIN = r"""
#include <cstdio>
#include "%s"
// prints the constants, then one line per L = 0..HMCG_ACF_MAXLAG: lags_r lag_threads groups group_draws work_doubles
int main()
{
    using namespace hmcg_host;
    std::printf("%%lld %%d %%d %%d %%d\n", PRED_SLAB, ACF_NT, ACF_J, ACF_SUMS, HMCG_ACF_MAXLAG);
    for (int L = 0; L <= HMCG_ACF_MAXLAG; ++L) {
        const AcfPlan p = acf_plan(L);
        std::printf("%%d %%d %%d %%d %%lld\n", p.lags_r, p.lag_threads, p.groups, p.group_draws, acf_work_doubles(L));
    }
    std::printf("%%lld %%lld %%lld %%lld\n", acf_pre(0, 1024), acf_pre(1024, 1024), acf_pre(1024, 17), acf_pre(2048, 0));
    return 0;
}
"""


def _plan(L):
    """autocorr_plan.hpp's acf_plan and acf_work_doubles, restated."""
    lags_r = (L + 8) // 8 * 8
    lt = 2
    while lt * 8 < L + 1:
        lt *= 2
    return [lags_r, lt, 256 // lt, 1024 // (256 // lt), (L + 1) + 6 + 1 + 2 * L]


def test_plan_header_against_a_restatement(tmp_path):
    """csrc/autocorr_plan.hpp, compiled by g++ -Wall -Werror into a stand-alone program and once more with
    -fsanitize=address,undefined: the split of the 256 threads over lags and draws for every L against the Python
    restatement, and the properties the kernel relies on -- every lag 0..L has a thread, the halo covers the window of the last
    lag thread, the shares tile the slab in whole register tiles, the staged draws fit the kernel's LDS array."""
    src = tmp_path / "plan_main.cpp"
    src.write_text(PLAN_MAIN % os.path.join(ROOT, "hmc.jl_amd", "csrc", "autocorr_plan.hpp"))
    exe, san = tmp_path / "plan_main", tmp_path / "plan_main_san"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", str(src), "-o", str(exe)])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           str(src), "-o", str(san)])
    out = subprocess.check_output([str(exe)]).decode().splitlines()
    assert subprocess.check_output([str(san)]).decode().splitlines() == out
    assert out[0].split() == ["1024", "256", "8", "6", "1024"] and _lib.PRED_SLAB == 1024
    assert len(out) == 1 + 1025 + 1
    for L in range(1025):
        got = [int(v) for v in out[1 + L].split()]
        assert got == _plan(L), (L, got)
        lags_r, lt, groups, gd, _ = got
        assert lt * 8 >= L + 1 and lt * groups == 256 and groups * gd == 1024 and gd % 8 == 0 and gd >= 8
        assert lags_r % 8 == 0 and L + 1 <= lags_r <= L + 8
        l0_max = L // 8 * 8                                  # the last lag thread that works
        assert l0_max // 8 < lt and l0_max + 8 <= lags_r      # its window starts at most lags_r draws before the share
        assert 1024 + lags_r <= 1024 + 1032
    assert [_plan(L)[1] for L in (0, 15, 16, 255, 256, 1023, 1024)] == [2, 2, 4, 32, 64, 128, 256]
    assert out[-1].split() == ["0", "1024", "17", "0"]


def test_ar1_chains_recover_the_integrated_autocorrelation_time():
    """The reference alone, seeded: AR(1) chains with phi in {0, 0.5, 0.9, -0.5}, n = 50 000, L = 199, and phi = 0.5 offset by
    1e4.  tau lies within 10 % of (1 + phi) / (1 - phi), the sequence stops by itself (truncated = 0), ess = n / tau, the offset
    costs no digits, and no pair sum up to the stop lies near zero (the GPU test relies on that)."""
    x, ref = ac.ar1_suite()
    want = np.array([(1 + phi) / (1 - phi) for phi in ac.AR1_PHIS])
    assert (np.abs(ref["tau"][0] - want) <= 0.1 * want).all(), (ref["tau"], want)
    assert not ref["truncated"].any() and (ref["pairs"] >= 1).all() and (ref["pairs"] < 100).all()
    assert np.array_equal(ref["ess"], ac.AR1_N / ref["tau"])
    assert np.allclose(ref["mcse"], np.sqrt(ref["variance"].astype(float) * ref["tau"] / ac.AR1_N), rtol=1e-14, atol=0)
    for c in range(len(ac.AR1_PHIS)):
        assert min(abs(P) for P in ref["P"][0][c]) > 1e-6
    # acov_0 is the biased variance, and the acov of an AR(1) chain decays like phi^l
    a = ref["acov"][0].astype(float)
    assert np.allclose(a[:, 0], ref["variance"][0].astype(float) * (ac.AR1_N - 1) / ac.AR1_N, rtol=1e-12, atol=0)
    assert abs(a[2, 1] / a[2, 0] - 0.9) < 0.01 and abs(a[3, 1] / a[3, 0] + 0.5) < 0.01
    # the offset chain against the same chain without the offset: the pivot takes the offset out before any product
    plain = ac.reference(x[:, 4:5] - 1e4, ac.AR1_LAGS, False)
    assert np.allclose(plain["acov"].astype(float), ref["acov"][:, 4:5].astype(float), rtol=1e-7, atol=0)
    assert plain["pairs"][0, 0] == ref["pairs"][0, 4] and abs(plain["tau"][0, 0] - ref["tau"][0, 4]) < 1e-6
    # the bound of the tolerance is near 1e-11 relative to acov_0
    rel = ref["acov_bound"][0, :, 0] / a[:, 0]
    assert (rel > 1e-12).all() and (rel < 1e-9).all()


def test_reference_acov_is_the_textbook_autocovariance():
    """The pivoted form of include/hmcg.h equals sum (x_d - mean)(x_(d-l) - mean) / n, computed directly in long double; the
    restated device sums agree with plain sums to rounding; the fp64 file route of hmc agrees within the derived bound."""
    x = ac.make_case(3, 2, 4, 700)
    ref = ac.reference(x, 64, False)
    xs = x.astype(ac.LD)
    mean = xs.mean(axis=2, keepdims=True)
    dev = xs - mean
    direct = np.stack([(dev[:, :, l:] * dev[:, :, :700 - l]).sum(axis=2) / 700 for l in range(65)], axis=2)
    scale = np.abs(direct[:, :, :1]).astype(float)
    assert (np.abs((direct - ref["acov"]).astype(float)) <= 1e-13 * np.maximum(scale, (1e-4) ** 2 * 1e8)).all()
    _, p, a = ac.prepare(x, False)
    mean2, var2, rhat2 = ac.moments_of_sums(ac.device_sums(a), p, 700)
    tol = ac.tolerance(ref)
    assert (np.abs(mean2 - ref["mean"].astype(float)) <= tol["mean"]).all() and (np.abs(var2 - ref["variance"].astype(float)) <= tol["variance"]).all()
    assert np.allclose(rhat2, ref["rhat"].astype(float), rtol=1e-10, atol=0)
    for w in range(2):
        parts = hmc._autocorr_from_cells(np.ascontiguousarray(x[w].T), 64)
        assert (np.abs(parts["acov"] - ref["acov"][w].astype(float)) <= tol["acov"][w]).all()
        assert np.array_equal(parts["pairs"], ref["pairs"][w]) and np.array_equal(parts["truncated"], ref["truncated"][w])


def test_split_rhat_on_white_noise_and_on_a_shifted_chain():
    rng = np.random.default_rng(21)
    n = 20000
    white = rng.standard_normal((1, 3, n))
    ref = ac.reference(white, 50, False)
    assert (np.abs(ref["rhat"].astype(float) - 1.0) < 0.01).all()
    shifted = white.copy()
    shifted[:, :, n // 2:] += 1.0                            # the halves disagree by one standard deviation
    ref = ac.reference(shifted, 50, False)
    assert (ref["rhat"].astype(float) > 1.1).all()
    _, p, a = ac.prepare(shifted, False)
    assert (ac.moments_of_sums(ac.device_sums(a), p, n)[2] > 1.1).all()
    # nothing is special-cased: too few draws or a constant column give NaN
    assert np.isnan(ac.reference(white[:, :, :3], 1, False)["rhat"].astype(float)).all()
    const = ac.reference(np.full((1, 1, 100), 2.5), 10, False)
    assert np.isnan(const["rhat"].astype(float)).all() and (const["acov"] == 0).all() and const["pairs"][0, 0] == 0
    assert np.isnan(const["tau"]).all() and not const["truncated"].any() and (const["acov_bound"] == 0).all()
    # an odd n with a NaN exactly between the halves still reaches rhat
    odd = white[:, :1, :101].copy()
    odd[0, 0, 50] = np.nan
    _, p, a = ac.prepare(odd, False)
    assert np.isnan(ac.moments_of_sums(ac.device_sums(a), p, 101)[2]).all() and np.isnan(ac.reference(odd, 5, False)["rhat"].astype(float)).all()
    # a lag window too short for the chain
    slow = ac.reference(ac.ar1(11, 0.99, 4096)[None, None, :], 15, False)
    assert slow["truncated"][0, 0] and slow["pairs"][0, 0] == 8
    assert ac.reference(white[:, :, :10], 0, False)["truncated"].all()        # L = 0 has no pair at all


def _hand_made(seed, K=3, n=300):
    """Draws in the reference's Julia shapes: means, variances, states (n, K), A (n, K, K) with A[d, i, j]; the means follow an
    AR(1) chain so that the diagnostics have something to find."""
    rng = np.random.default_rng(seed)
    means = np.stack([ac.ar1(seed * 10 + k, 0.6, n, 3.0 * k, 0.5) for k in range(K)], axis=1)
    variances = 0.05 + rng.gamma(2.0, 0.8, size=(n, K))
    states = rng.dirichlet(np.ones(K), size=n)
    A = rng.dirichlet(np.ones(K) * 2.0, size=(n, K))
    return means, variances, states, A


def test_calcess_file_route_and_writer(tmp_path):
    """Per-draw files written by hmc.saveresults from hand-made draws (K = 3, n = 300, two dates) through hmc.calcess (numpy, no
    GPU) against autocorr_cases.reference on the same draws, rounded as the cells are; then the writer's text."""
    dates = [dt.date(1980, 1, 1), dt.date(1985, 1, 1)]
    draws = [_hand_made(41 + i) for i in range(2)]
    for d, (means, variances, states, A) in zip(dates, draws):
        n, K = means.shape
        ds = [dt.date(1960 + i // 12, i % 12 + 1, 1) for i in range(11)] + [d]
        opt = hmc.estopt(np.zeros(12), ds, sampleRange=range(1, 13), endIndex=12, horizons=(12,), D=K, burnin=1, Nrun=n)
        hmc.saveresults(hmc.Samples(means, variances, states[:, None, :], A, np.zeros((n, 2)), [d] * n), opt, str(tmp_path), native=False)
    abi = {"mu": np.stack([m.T for m, _, _, _ in draws]), "sig2": np.stack([v.T for _, v, _, _ in draws]),
           "A": np.stack([np.transpose(a, (2, 1, 0)) for _, _, _, a in draws])}
    for var in ("mu", "sig2", "A"):
        got_dates, d = hmc.calcess(str(tmp_path), dates, var, 40)
        assert got_dates == [str(x) for x in dates] and d.lags == 40 and d.var == var
        assert d.columns == (["trans_%d_%d" % (i, j) for j in (1, 2, 3) for i in (1, 2, 3)] if var == "A" else ["state_1", "state_2", "state_3"])
        ref = ac.reference(abi[var], 40, True)
        tol = ac.tolerance(ref)
        Cn = len(d.columns)
        assert d.acov.shape == (2, Cn, 41) and d.pairs.dtype == np.int64 and d.truncated.dtype == bool
        for k in ("acov", "mean", "variance"):
            assert (np.abs(getattr(d, k).astype(ac.LD) - ref[k]).astype(float) <= tol[k]).all(), (var, k)
        assert np.array_equal(d.pairs, ref["pairs"]) and np.array_equal(d.truncated, ref["truncated"])
        assert np.allclose(d.tau, ref["tau"], rtol=1e-10, atol=0) and np.allclose(d.ess, 300 / d.tau, rtol=1e-14, atol=0)
        assert np.allclose(d.rhat, ref["rhat"].astype(float), rtol=1e-10, atol=0)
    _, mu = hmc.calcess(str(tmp_path), dates, "mu", 40)
    assert (mu.tau > 2.0).all() and (mu.tau < 8.0).all()               # phi = 0.6: tau = 4
    one = mu.rows([1])
    assert one.acov.shape == (1, 3, 41) and np.array_equal(one.tau, mu.tau[1:])
    with pytest.raises(FileNotFoundError):
        hmc.calcess(str(tmp_path), [dt.date(1990, 1, 1)])
    with pytest.raises(ValueError, match="lags = 300"):
        hmc.calcess(str(tmp_path), dates, "mu", 300)
    with pytest.raises(ValueError, match="var must be"):
        hmc.calcess("unused", [], "x")
    path = hmc.write_chain_ess(str(tmp_path / "chain_ess.csv"), [str(x) for x in dates], mu)
    header, rows = hmc._read_csv(path)
    assert header == ["date", "column", "mean", "variance", "tau", "ess", "mcse", "pairs", "truncated", "rhat"] and len(rows) == 2 * 3
    r = rows[1 * 3 + 2]
    assert r[:2] == ["1985-01-01", "state_3"] and r[4] == hmc._fmt(mu.tau[1, 2]) and r[5] == hmc._fmt(mu.ess[1, 2])
    assert r[7] == str(int(mu.pairs[1, 2])) and r[8] == "0" and r[9] == hmc._fmt(mu.rhat[1, 2])


def test_batchresult_autocorr_is_none_unless_asked_for():
    res = hmc.BatchResult([], {"summary": np.zeros((0, 1)), "status": np.zeros(0, dtype=np.int32)}, False)
    assert res.autocorr is None
    with pytest.raises(ValueError, match="no autocorrelation"):
        hmc.calcess("unused", ["1980-01-01"], "mu", result=res)
    empty = {"acov": np.zeros((0, 3, 9)), "pairs": np.zeros((0, 3), dtype=np.int64), "truncated": np.zeros((0, 3), dtype=bool)}
    empty.update({k: np.zeros((0, 3)) for k in ("mean", "variance", "tau", "ess", "mcse", "rhat")})
    res.autocorr = {"mu": hmc.ChainAutocorr("mu", ["state_1", "state_2", "state_3"], empty)}
    with pytest.raises(ValueError, match="no autocorrelation of sig2"):
        hmc.calcess("unused", [], "sig2", result=res)
    with pytest.raises(ValueError, match="other lags"):
        hmc.calcess("unused", [], "mu", 16, result=res)
    assert hmc.calcess("unused", [], "mu", 8, result=res)[1].acov.shape == (0, 3, 9)
    with pytest.raises(ValueError, match="acf_vars"):
        hmc.estimatewindows(np.zeros(30), [dt.date(2000, 1, 1)] * 30, [20], acf_vars=("x",))
    out = _lib.unpack_chain_autocorr(np.zeros((2, 3, 5)), np.arange(48.0).reshape(2, 3, 8))
    assert out["pairs"].dtype == np.int64 and out["truncated"].dtype == bool and out["rhat"][1, 2] == 47.0 and out["pairs"][0, 1] == 13
