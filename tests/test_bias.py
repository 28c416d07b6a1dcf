"""Uncertainty-bias moments of the draws (hmcg_bias_moments, bias_calcs.jl): the parts that need no GPU -- the struct and the
argument rules of the built library (checked before device init), csrc/bias_plan.hpp run by a g++-compiled program, and the
host-side file route of hmc.calcbias against the longdouble reference, the index swap of `uncbias` included."""
import ctypes as C
import datetime as dt
import os
import subprocess

import numpy as np
import pytest

import hmc_jl_amd
from hmc_jl_amd import _lib, hmc

import bias_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ctypes_struct_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "%s"\nint main(void){printf("%%zu %%d %%d %%d %%d %%d", sizeof(hmcg_bias), '
                   'HMCG_BIAS_ROUND5, HMCG_BIAS_STRIDE(2), HMCG_BIAS_STRIDE(3), HMCG_BIAS_STRIDE(8), HMCG_VERSION);return 0;}\n'
                   % os.path.join(ROOT, "include", "hmcg.h"))
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.Bias), _lib.BIAS_ROUND5, _lib.bias_stride(2), _lib.bias_stride(3), _lib.bias_stride(8), 109]
    assert [_lib.bias_stride(K) for K in (2, 3, 8)] == [22, 44, 274]
    assert hmc_jl_amd.load().hmcg_version() == 109


MISUSE = [
    (dict(struct_size=7), {}, b"struct_size"),
    (dict(K=1), {}, b"K = 1"),
    (dict(K=9), {}, b"K = 9"),
    (dict(horizon=-1), {}, b"horizon -1"),
    (dict(horizon=_lib.HMCG_PRED_MAXH + 1), {}, b"horizon 1025"),
    (dict(W=0), {}, b"at least one window"),
    (dict(nd=0), {}, b"at least one draw"),
    (dict(nd_ld=3), {}, b"nd_ld"),
    ({}, dict(mu=False), b"required"),
    ({}, dict(pi_end=False), b"required"),
    ({}, dict(out=False), b"required"),
    ({}, dict(A=False), b"A is NULL"),
    (dict(H=0), {}, b"fcast given with H = 0"),
    (dict(H=_lib.HMCG_MAXH + 1), {}, b"fcast given with H = 9"),
]


@pytest.mark.parametrize("entry", ["hmcg_bias_moments", "hmcg_bias_moments_device"])
def test_misuse_is_refused_before_device_init(entry):
    """Every rule returns HMCG_E_BADARG with its text from the built library; the pointers are never followed (the device entry is
    handed host addresses here) and no GPU is needed: the check precedes get_context."""
    lib = hmc_jl_amd.load()
    buf = np.zeros(64)
    ok = C.c_void_p(buf.ctypes.data)
    for fields, ptrs, text in MISUSE:
        p = _lib.make_bias(1, 3, 4, 4, 12, 1)
        for k, v in fields.items():
            setattr(p, k, v)
        a = {n: (ok if ptrs.get(n, True) else None) for n in ("mu", "pi_end", "A", "fcast", "out")}
        args = [C.byref(p), a["mu"], a["pi_end"], a["A"], a["fcast"], a["out"]] + ([None] if entry.endswith("device") else []) + [None]
        rc = getattr(lib, entry)(*args)
        assert rc == -1 and text in lib.hmcg_last_error(), (fields, ptrs, rc, lib.hmcg_last_error())


# Two rules broken at once: the rule the entry names first, with its whole text.  The order is this feature's own (the horizon
# stands between K and nd); the texts of the rules it shares with the other draw statistics come from csrc/stat_plan.hpp.
DOUBLY_WRONG = [
    (dict(struct_size=7, W=0), b"hmcg_bias.struct_size 7 != %d" % C.sizeof(_lib.Bias)),
    (dict(W=0, nd_ld=3), b"W = 0: at least one window"),
    (dict(K=9, nd=0), b"K = 9 outside 2..8"),
    (dict(horizon=-1, nd=0), b"horizon -1 outside 0..1024"),
    (dict(nd=0, nd_ld=-1), b"nd = 0: at least one draw"),
    (dict(nd_ld=3, H=0), b"nd_ld = 3 < nd = 4"),
]


@pytest.mark.parametrize("fields, message", DOUBLY_WRONG)
@pytest.mark.parametrize("entry", ["hmcg_bias_moments", "hmcg_bias_moments_device"])
def test_first_rule_named_for_a_doubly_wrong_call(entry, fields, message):
    lib = hmc_jl_amd.load()
    buf = np.zeros(64)
    ok = C.c_void_p(buf.ctypes.data)
    p = _lib.make_bias(1, 3, 4, 4, 12, 1)
    for k, v in fields.items():
        setattr(p, k, v)
    rc = getattr(lib, entry)(C.byref(p), ok, ok, ok, ok, ok, *(([None] if entry.endswith("device") else []) + [None]))
    assert rc == -1 and lib.hmcg_last_error() == message


PLAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "%s"
int main(int argc, char** argv)
{
    using namespace hmcg_host;
    std::printf("%%lld\n", PRED_SLAB);
    for (int K = 2; K <= HMCG_MAXK; ++K) std::printf("%%d %%d %%d %%d\n", K, bias_vars(K), bias_items(K), (int)HMCG_BIAS_STRIDE(K));
    hmcg_bias p{};
    p.struct_size = (int32_t)sizeof p; p.W = 3; p.K = 3; p.nd = p.nd_ld = 5; p.horizon = 12; p.H = 1;
    char msg[160] = "";
    const double x[2] = {0.0, 1.0};
    std::printf("%%d %%d %%d\n", check_bias(&p, x, x, x, x, x, msg, sizeof msg), bias_columns(p, true), bias_columns(p, false));
    std::printf("%%d %%s\n", check_bias(&p, x, x, nullptr, x, x, msg, sizeof msg), msg);
    p.horizon = 0;
    std::printf("%%d %%d %%d\n", check_bias(&p, x, x, nullptr, nullptr, x, msg, sizeof msg), bias_columns(p, true), bias_columns(p, false));
    p.H = 0;
    std::printf("%%d %%s\n", check_bias(&p, x, x, nullptr, x, x, msg, sizeof msg), msg);
    std::printf("%%d %%s\n", check_bias(nullptr, x, x, x, x, x, msg, sizeof msg), msg);
    for (int i = 1; i + 2 < argc; i += 3) {
        const long long nd = std::atoll(argv[i]), cap = std::atoll(argv[i + 1]);
        const int ncol = std::atoi(argv[i + 2]);
        const long long cd = pred_chunk_draws(nd, 3, ncol, cap);
        std::printf("%%lld %%lld %%lld %%lld :", nd, cap, pred_slabs(nd), cd);
        for (const PredChunk& c : pred_chunks(nd, cd)) std::printf(" %%lld+%%lld", c.d0, c.n);
        std::printf("\n");
    }
    return 0;
}
"""


def test_plan_header_rules_columns_and_chunk_cuts(tmp_path):
    """csrc/bias_plan.hpp, compiled by g++ into a stand-alone program: the argument rules, the item and column counts, and the
    chunk cut it shares with the predictive CDFs at this feature's column counts (16 with A and the forecast error at K = 3, 6
    without): whole slabs, on slab boundaries, covering [0, nd) once."""
    S = _lib.PRED_SLAB
    src = tmp_path / "plan_main.cpp"
    src.write_text(PLAN_MAIN % os.path.join(ROOT, "hmc.jl_amd", "csrc", "bias_plan.hpp"))
    exe = tmp_path / "plan_main"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", str(src), "-o", str(exe)])
    table = [(1, 0, 16), (S, 0, 16), (S + 1, 1, 16), (3 * S + 17, S + 476, 16), (3 * S + 17, 1, 16), (3 * S + 17, 0, 6), (250000, 0, 16),
             (250000, 10000, 6)]
    out = subprocess.check_output([str(exe)] + [str(v) for row in table for v in row]).decode().splitlines()
    assert int(out[0]) == S == 1024
    for K, line in zip(range(2, 9), out[1:8]):
        assert [int(v) for v in line.split()] == [K, 2 * K, K * (2 * K + 1) + 2 * K + 1, 2 + 2 * K + 4 * K * K]
    assert out[8].split() == ["0", "16", "15"]
    assert out[9].startswith("-1 A is NULL")
    assert out[10].split() == ["0", "7", "6"]
    assert out[11].startswith("-1 fcast given with H = 0")
    assert out[12].startswith("-1 hmcg_bias is NULL")
    for (nd, cap, ncol), line in zip(table, out[13:]):
        head, _, tail = line.partition(":")
        nd_, cap_, nslab, cd = [int(v) for v in head.split()]
        assert (nd_, cap_) == (nd, cap) and nslab == -(-nd // S) and cd % S == 0 and cd >= S
        if 0 < cap < nd:
            assert cd == -(-cap // S) * S
        chunks = [tuple(int(v) for v in c.split("+")) for c in tail.split()]
        pos = 0
        for i, (d0, n) in enumerate(chunks):
            assert d0 == pos and d0 % S == 0 and 1 <= n <= cd and (n % S == 0 or i == len(chunks) - 1)
            pos += n
        assert pos == nd
    assert len(out[13 + 3].partition(":")[2].split()) == 2 and len(out[13 + 4].partition(":")[2].split()) == 4


def _hand_made(seed, K=3, n=300, spread=1.0):
    """Draws in the reference's Julia shapes: means (n, K), states (n, K), A (n, K, K) with A[d, i, j], forecasts (n, 2)."""
    rng = np.random.default_rng(seed)
    means = np.sort(rng.normal(3.0, 2.5 * spread, size=(n, K)), axis=1)
    states = rng.dirichlet(np.ones(K), size=n)
    A = rng.dirichlet(np.ones(K) * 2.0, size=(n, K))
    fc = rng.normal(0.4, 1.2, size=(n, 2))
    return means, states, A, fc


def _save(tmp_path, date, means, states, A, fc):
    n, K = means.shape
    dates = [dt.date(1960 + i // 12, i % 12 + 1, 1) for i in range(11)] + [date]
    opt = hmc.estopt(np.zeros(12), dates, sampleRange=range(1, 13), endIndex=12, horizons=(12,), D=K, burnin=1, Nrun=n)
    s = hmc.Samples(means, 1.0 + np.zeros_like(means), states[:, None, :], A, fc, [date] * n)
    hmc.saveresults(s, opt, str(tmp_path))


def _abi(means, states, A, fc):
    return means.T[None].copy(), states.T[None].copy(), np.transpose(A, (2, 1, 0))[None].copy(), fc.T[None].copy()


def test_calcbias_file_route_against_the_reference(tmp_path):
    """Files written by hmc.saveresults from hand-made draws (K = 3, n = 300, two dates) through hmc.calcbias (numpy, no GPU)
    against bias_cases.reference on the same draws, rounded as the cells are."""
    dates = [dt.date(1980, 1, 1), dt.date(1985, 1, 1)]
    draws = [_hand_made(21 + i) for i in range(2)]
    for d, dr in zip(dates, draws):
        _save(tmp_path, d, *dr)
    got_dates, unc, tot, mean, cov = hmc.calcbias(str(tmp_path), dates, 12)
    assert got_dates == [str(d) for d in dates] and unc.shape == tot.shape == (2,) and mean.shape == (2, 6) and cov.shape == (2, 6, 6)
    for i, dr in enumerate(draws):
        ref = bc.reference(*_abi(*dr), 12, True)
        tol = bc.tolerance(ref, 300, 3, 12)
        bc.check({"uncbias": unc[i:i + 1], "totalbias": tot[i:i + 1], "mean": mean[i:i + 1], "cov": cov[i:i + 1]}, ref, tol, "files %d" % i)
        assert np.isfinite(unc[i]) and np.isfinite(tot[i])
        # totalbias is the mean of the forecast_error cells of the FIRST horizon (forecasts[:, 3] upstream)
        assert abs(tot[i] - np.mean(np.round(dr[3][:, 1], 5))) <= 300 * 2.0 ** -52 * np.abs(dr[3][:, 1]).max()
    # another horizon gives other numbers, horizon 0 uses the state probabilities themselves
    _, unc0, tot0, mean0, _ = hmc.calcbias(str(tmp_path), dates[:1], 0)
    assert tot0[0] == tot[0] and unc0[0] != unc[0]
    assert np.abs(mean0[0, :3] - np.round(draws[0][1], 5).mean(axis=0)).max() < 1e-15
    with pytest.raises(FileNotFoundError):
        hmc.calcbias(str(tmp_path), [dt.date(1990, 1, 1)])


def test_uncbias_keeps_the_reference_index_swap(tmp_path):
    """nab is ordered means | futstate, covv futstate | means (bias_calcs.jl:49-50).  With means of a few units and state
    probabilities below one the two blocks differ clearly: the file route equals the swapped form and is far from the aligned
    one, which the returned mean and cov give in one line."""
    d = dt.date(1990, 1, 1)
    dr = _hand_made(5)
    _save(tmp_path, d, *dr)
    _, unc, _, mean, cov = hmc.calcbias(str(tmp_path), [d], 12)
    ref = bc.reference(*_abi(*dr), 12, True)
    tol = bc.tolerance(ref, 300, 3, 12)
    m, c = ref["mean"][0], ref["cov"][0]
    swapped = np.concatenate([m[3:], m[:3]])
    assert abs(np.longdouble(unc[0]) - swapped @ c @ swapped) <= tol["uncbias"][0]
    assert abs(ref["uncbias"][0] - swapped @ c @ swapped) <= 1e-17
    aligned = float(m @ c @ m)
    assert abs(unc[0] - aligned) > 1e6 * tol["uncbias"][0] and abs(unc[0] - aligned) > 1e-3
    assert abs(float(mean[0] @ cov[0] @ mean[0]) - aligned) <= 4 * tol["uncbias"][0]


def test_reference_and_tolerance_basics():
    """The helpers themselves: n = 1 gives NaN cov and uncbias and a finite mean; identical draws give a zero bound; the bound
    scales with the spread about draw 0 and not with a common offset (the point of the pivot)."""
    mu, pi, A, fc = bc.make_draws(3, 2, 3, 40, 5, True, 2)
    one = bc.reference(mu, pi, A, fc, 12, True, 1)
    assert np.isnan(one["cov"]).all() and np.isnan(one["uncbias"]).all() and np.isfinite(one["mean"]).all() and np.isfinite(one["totalbias"]).all()
    assert np.isnan(bc.reference(mu, pi, A, None, 12, True, 40)["totalbias"]).all()
    ref = bc.reference(mu, pi, A, fc, 12, True, 40)
    assert np.isfinite(ref["cov"]).all() and np.array_equal(ref["cov"], np.transpose(ref["cov"], (0, 2, 1)))
    same = [np.repeat(a[..., :1], 40, axis=-1) for a in (mu, pi, A, fc)]
    r0 = bc.reference(*same, 12, True)
    assert (bc.tolerance(r0, 40, 3, 12)["cov"] == 0.0).all() and (r0["R"] == 0).all()
    shifted = bc.reference(mu + 1e4, pi, A, fc, 12, False, 40)
    plain = bc.reference(mu, pi, A, fc, 12, False, 40)
    t1, t0 = bc.tolerance(shifted, 40, 3, 12)["cov"], bc.tolerance(plain, 40, 3, 12)["cov"]
    assert np.abs(t1 - t0).max() <= 1e-3 * t0.max()


def test_batchresult_bias_is_none_unless_asked_for():
    res = hmc.BatchResult([], {"summary": np.zeros((0, 1)), "status": np.zeros(0, dtype=np.int32)}, False)
    assert res.bias is None
    with pytest.raises(ValueError, match="no bias moments"):
        hmc.calcbias("unused", ["1980-01-01"], result=res)
    res.bias = hmc.BiasMoments(6, np.zeros(0), np.zeros(0), np.zeros((0, 6)), np.zeros((0, 6, 6)))
    with pytest.raises(ValueError, match="another horizon"):
        hmc.calcbias("unused", [], 12, result=res)


def test_write_biases(tmp_path):
    path = hmc.write_biases(str(tmp_path / "biases.csv"), ["1980-01-01", "1981-01-01"], [0.5, float("nan")], [-2.0, 2.4e-10])
    assert open(path).read().splitlines() == ["date,uncerbias,totalbias", "1980-01-01,0.5,-2", "1981-01-01,NaN,24e-11"]
