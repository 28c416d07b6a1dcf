"""Predictive-mixture moments of the draws (hmcg_mixture_moments; skewness.jl and alt_forecasts.jl): the parts that need no GPU
-- the struct and the argument rules of the built library (checked before device init), csrc/mixmoments_plan.hpp run by a
g++-compiled program, the closed forms of the reference against sampling, hmc.calcskewness and hmc.altforecasts on the
committed official summaries, and the host-side file route of hmc.calcmoments against the longdouble reference."""
import ctypes as C
import datetime as dt
import os
import shutil
import subprocess

import numpy as np
import pytest

import hmc_jl_amd
from hmc_jl_amd import _lib, hmc

import mixmoments_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LD = np.longdouble


def test_ctypes_struct_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "%s"\nint main(void){printf("%%zu %%d %%d %%d %%d", sizeof(hmcg_mixmom), '
                   'HMCG_MIX_ROUND5, HMCG_MIX_STRIDE, HMCG_MAXH, HMCG_VERSION);return 0;}\n' % os.path.join(ROOT, "include", "hmcg.h"))
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:4] == [C.sizeof(_lib.MixMom), _lib.MIX_ROUND5, _lib.MIX_STRIDE, _lib.HMCG_MAXH]
    assert _lib.MIX_STRIDE == 8 == len(_lib.MIX_FIELDS) and C.sizeof(_lib.MixMom) == 72
    assert hmc_jl_amd.load().hmcg_version() == got[4]                     # the header and the library agree
    assert {"hmcg_mixture_moments", "hmcg_mixture_moments_device"} <= set(_lib.EXPORTS)


MISUSE = [
    (dict(struct_size=7), {}, b"struct_size"),
    (dict(K=1), {}, b"K = 1"),
    (dict(K=9), {}, b"K = 9"),
    (dict(n_h=0), {}, b"n_h = 0"),
    (dict(n_h=_lib.HMCG_MAXH + 1), {}, b"n_h = 9"),
    (dict(h1=-1), {}, b"horizon -1"),
    (dict(h1=_lib.HMCG_PRED_MAXH + 1), {}, b"horizon 1025"),
    (dict(W=0), {}, b"at least one window"),
    (dict(nd=0), {}, b"at least one draw"),
    (dict(nd_ld=3), {}, b"nd_ld"),
    ({}, dict(mu=False), b"required"),
    ({}, dict(sig2=False), b"required"),
    ({}, dict(pi_end=False), b"required"),
    ({}, dict(out=False), b"required"),
    ({}, dict(A=False), b"A is NULL"),
]


@pytest.mark.parametrize("entry", ["hmcg_mixture_moments", "hmcg_mixture_moments_device"])
def test_misuse_is_refused_before_device_init(entry):
    """Every rule returns HMCG_E_BADARG with its text from the built library; the pointers are never followed (the device entry is
    handed host addresses here) and no GPU is needed: the check precedes get_context."""
    lib = hmc_jl_amd.load()
    buf = np.zeros(64)
    ok = C.c_void_p(buf.ctypes.data)
    for fields, ptrs, text in MISUSE:
        p = _lib.make_mixmom(1, 3, 4, 4, (0, 12))
        for k, v in fields.items():
            if k == "h1":
                p.horizons[1] = v
            else:
                setattr(p, k, v)
        a = {n: (ok if ptrs.get(n, True) else None) for n in ("mu", "sig2", "pi_end", "A", "out")}
        args = [C.byref(p), a["mu"], a["sig2"], a["pi_end"], a["A"], a["out"]] + ([None] if entry.endswith("device") else []) + [None]
        rc = getattr(lib, entry)(*args)
        assert rc == -1 and text in lib.hmcg_last_error(), (fields, ptrs, rc, lib.hmcg_last_error())
    with pytest.raises(ValueError, match="at most 8 horizons"):
        _lib.make_mixmom(1, 3, 4, 4, tuple(range(9)))


# Two rules broken at once: the rule the entry names first, with its whole text.  The order is this feature's own (the horizons
# stand between K and nd); the texts of the rules it shares with the other draw statistics come from csrc/stat_plan.hpp.
DOUBLY_WRONG = [
    (dict(struct_size=7, W=0), b"hmcg_mixmom.struct_size 7 != %d" % C.sizeof(_lib.MixMom)),
    (dict(W=0, nd_ld=3), b"W = 0: at least one window"),
    (dict(K=9, nd=0), b"K = 9 outside 2..8"),
    (dict(n_h=9, nd_ld=3), b"n_h = 9 horizons outside 1..8"),
    (dict(h1=-1, nd=0), b"horizon -1 outside 0..1024"),
    (dict(nd=0, nd_ld=-1), b"nd = 0: at least one draw"),
]


@pytest.mark.parametrize("fields, message", DOUBLY_WRONG)
@pytest.mark.parametrize("entry", ["hmcg_mixture_moments", "hmcg_mixture_moments_device"])
def test_first_rule_named_for_a_doubly_wrong_call(entry, fields, message):
    lib = hmc_jl_amd.load()
    buf = np.zeros(64)
    ok = C.c_void_p(buf.ctypes.data)
    p = _lib.make_mixmom(1, 3, 4, 4, (0, 12))
    for k, v in fields.items():
        if k == "h1":
            p.horizons[1] = v
        else:
            setattr(p, k, v)
    rc = getattr(lib, entry)(C.byref(p), ok, ok, ok, ok, ok, *(([None] if entry.endswith("device") else []) + [None]))
    assert rc == -1 and lib.hmcg_last_error() == message


PLAN_MAIN = r"""
#include <cstdio>
#include "%s"
int main()
{
    using namespace hmcg_host;
    std::printf("%%d %%d %%lld\n", MIX_ITEMS, MIX_PIVOTS, PRED_SLAB);
    hmcg_mixmom p{};
    p.struct_size = (int32_t)sizeof p; p.W = 3; p.K = 3; p.nd = p.nd_ld = 5; p.n_h = 8;
    const int hs[8] = {12, 0, 3, 1, 12, 7, 2, 5};
    for (int j = 0; j < 8; ++j) p.horizons[j] = hs[j];
    char msg[160] = "";
    const double x[2] = {0.0, 1.0};
    std::printf("%%d %%d %%d\n", check_mixmom(&p, x, x, x, x, x, msg, sizeof msg), mix_columns(p), mix_max_horizon(p));
    MixWalk w = mix_walk(p);
    for (int i = 0; i < 8; ++i) std::printf("%%d:%%d ", w.hz[i], w.slot[i]);
    std::printf("\n%%d %%s\n", check_mixmom(&p, x, x, x, nullptr, x, msg, sizeof msg), msg);
    p.n_h = 3; p.horizons[0] = 0; p.horizons[1] = 0; p.horizons[2] = 0;
    std::printf("%%d %%d %%d\n", check_mixmom(&p, x, x, x, nullptr, x, msg, sizeof msg), mix_columns(p), mix_max_horizon(p));
    w = mix_walk(p);
    for (int i = 0; i < 8; ++i) std::printf("%%d:%%d ", w.hz[i], w.slot[i]);
    p.K = 8; p.horizons[2] = 1;
    std::printf("\n%%d\n", mix_columns(p));
    p.horizons[1] = 1025;
    std::printf("%%d %%s\n", check_mixmom(&p, x, x, x, x, x, msg, sizeof msg), msg);
    std::printf("%%d %%s\n", check_mixmom(nullptr, x, x, x, x, x, msg, sizeof msg), msg);
    return 0;
}
"""


def test_plan_header_items_columns_walk_and_rules(tmp_path):
    """csrc/mixmoments_plan.hpp, compiled by g++ into a stand-alone program: nine slab sums per horizon, the column counts with
    and without A, the ascending walk with its permutation for unsorted and repeated horizons (stable: equal horizons keep
    their order), and the argument rules."""
    src = tmp_path / "plan_main.cpp"
    src.write_text(PLAN_MAIN % os.path.join(ROOT, "hmc.jl_amd", "csrc", "mixmoments_plan.hpp"))
    exe = tmp_path / "plan_main"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().splitlines()
    assert out[0].split() == ["9", "2", "1024"]
    assert out[1].split() == ["0", "18", "12"]                         # 3K + K^2 at K = 3
    assert out[2].split() == ["0:1", "1:3", "2:6", "3:2", "5:7", "7:5", "12:0", "12:4"]
    assert out[3].startswith("-1 A is NULL")
    assert out[4].split() == ["0", "9", "0"]                           # every horizon 0: A is neither needed nor counted
    assert out[5].split() == ["0:0", "0:1", "0:2"] + ["0:0"] * 5
    assert out[6].split() == ["88"]                                    # 3K + K^2 at K = 8
    assert out[7].startswith("-1 horizon 1025 outside 0..1024")
    assert out[8].startswith("-1 hmcg_mixmom is NULL")


def _sample_stats(rng, w, m, sd, N, B=100):
    """Mean, variance, skewness and excess kurtosis of N variates of the mixture sum w_i N(m_i, sd_i), each with its standard
    error estimated from the same sample (the spread of the statistic over B equal batches)."""
    idx = rng.choice(w.size, size=N, p=w / w.sum())
    x = rng.normal(m[idx], sd[idx])

    def stats(y):
        mu = y.mean()
        d = y - mu
        v = np.mean(d * d)
        return np.array([mu, v, np.mean(d ** 3) / v ** 1.5, np.mean(d ** 4) / (v * v) - 3.0])
    per = np.array([stats(b) for b in x.reshape(B, -1)])
    return stats(x), per.std(axis=0, ddof=1) / np.sqrt(B)


def test_closed_forms_against_sampling():
    """The pooled moments of the reference against 2e6 seeded variates of the nd K-component mixture itself, within 5 standard
    errors; then a one-hot mixture of identical draws, which is a single normal: variance v, skewness 0, excess kurtosis 0."""
    K, nd = 3, 50
    mu, sig2, pi, A = mc.make_draws(5, 1, K, nd)
    hz = (0, 12)
    ref = mc.reference(mu, sig2, pi, A, hz, False)
    rng = np.random.default_rng(2024)
    for j, h in enumerate(hz):
        w = mc.omegas(pi, A, h, np.float64)[0].reshape(-1)
        got, se = _sample_stats(rng, w, mu[0].reshape(-1), np.sqrt(sig2[0]).reshape(-1), 2_000_000)
        want = np.array([float(ref[k][0, j]) for k in ("mean", "variance", "skewness", "kurtosis")])
        print("h = %d: closed form %s, sample %s, standard errors %s" % (h, want, got, se))
        assert (np.abs(got - want) <= 5.0 * se).all() and (se > 0).all() and (se < 0.05 * np.abs(want[1])).all()
    assert abs(float(ref["skewness"][0, 0])) > 0.05                     # a skewed law: the check above can fail
    # the split: pooled variance = within + between when every draw has the same total weight (h = 0: exactly 1 here)
    assert abs(float(ref["variance"][0, 0] - ref["within"][0, 0] - ref["between"][0, 0])) < 1e-12
    hot = np.zeros_like(pi)
    hot[:, 1, :] = 1.0
    same = lambda a: np.repeat(a[..., :1], nd, axis=-1)
    one = mc.reference(same(mu), same(sig2), hot, None, (0,), False)
    tol = mc.tolerance(one, nd, K, (0,))
    assert float(one["variance"][0, 0]) == sig2[0, 1, 0] and float(one["mean"][0, 0]) == mu[0, 1, 0]
    assert abs(float(one["skewness"][0, 0])) <= tol["skewness"][0, 0] and abs(float(one["kurtosis"][0, 0])) <= tol["kurtosis"][0, 0]
    assert tol["skewness"][0, 0] < 1e-8 and tol["kurtosis"][0, 0] < 1e-8          # "0 within the bound" says something
    assert float(one["between"][0, 0]) == 0.0 and float(one["draw_skewness"][0, 0]) == 0.0


def test_reference_and_tolerance_basics():
    """nd = 1 is finite with between = 0; the bound scales with the spread about the pivot, not with a common offset; NaN draws
    give NaN bounds except for the weight."""
    mu, sig2, pi, A = mc.make_draws(3, 2, 3, 40, 5)
    one = mc.reference(mu, sig2, pi, A, (0, 12), True, 1)
    assert all(np.isfinite(one[k].astype(np.float64)).all() for k in mc.FIELDS) and (one["between"] == 0).all()
    plain = mc.reference(mu, sig2, pi, A, (12,), False, 40)
    shifted = mc.reference(mu + 1e4, sig2, pi, A, (12,), False, 40)
    t0, t1 = mc.tolerance(plain, 40, 3, (12,)), mc.tolerance(shifted, 40, 3, (12,))
    for k in mc.FIELDS[1:]:
        assert np.abs(t1[k] - t0[k]).max() <= 1e-3 * t0[k].max(), k
    assert (t0["variance"] < 1e-9).all() and (t0["skewness"] < 1e-9).all()         # against a variance near 10
    mu[0, 1, 7] = np.nan
    bad = mc.tolerance(mc.reference(mu, sig2, pi, A, (0,), True, 40), 40, 3, (0,))
    assert np.isnan(bad["mean"][0]).all() and np.isfinite(bad["mean"][1]).all() and np.isfinite(bad["weight"]).all()


def _official(tmp_path, stems):
    for s in stems:
        shutil.copy(os.path.join(GOLDEN, "official_%s_summary.csv" % s), tmp_path / ("%s_summary.csv" % s))
    return str(tmp_path)


def test_calcskewness_on_the_official_summaries(tmp_path):
    """hmc.calcskewness against skewness.jl's own recipe on the committed summaries: variates of the plug-in mixture of the
    latest date, ((x - mean(f)) / std(f))^3 averaged (seeded numpy, 4e6 instead of upstream's 1e7), within 5 standard errors."""
    d = _official(tmp_path, ("filtered_means", "filtered_variances", "filtered_state_probs"))
    date, mean, std, skew = hmc.calcskewness(d)
    assert date == "2018-03-01"
    rows = {s: hmc._read_csv(os.path.join(d, s + "_summary.csv"))[1][-1] for s in ("filtered_means", "filtered_variances", "filtered_state_probs")}
    assert all(r[0] == date for r in rows.values())
    m, v, p = (np.array([float(x) for x in rows[s][1:]]) for s in ("filtered_means", "filtered_variances", "filtered_state_probs"))
    p = p / p.sum()
    assert abs(mean - float(p @ m)) < 1e-14 and abs(std ** 2 - float(p @ (v + (m - mean) ** 2))) < 1e-13
    rng = np.random.default_rng(1)
    n = 4_000_000
    idx = rng.choice(3, size=n, p=p)
    cubes = ((rng.normal(m[idx], np.sqrt(v[idx])) - mean) / std) ** 3
    est, se = cubes.mean(), cubes.std(ddof=1) / np.sqrt(n)
    print("skewness of %s: closed form %.5f, sample %.5f +- %.5f" % (date, skew, est, se))
    assert abs(est - skew) <= 5.0 * se and se < 0.01
    assert abs(skew - 0.30801) < 5e-6
    first = hmc.calcskewness(d, "1979-12-01")
    assert first[0] == "1979-12-01" and first[3] != skew
    with pytest.raises(ValueError):
        hmc.calcskewness(d, "1900-01-01")


def test_altforecasts_on_the_official_summaries(tmp_path):
    """hmc.altforecasts / write_forecast_comparison against a longdouble recomputation on the committed summaries; the rows where
    the plug-in forecast leaves the proper one pin the column-major reshape of the transition row."""
    d = _official(tmp_path, ("filtered_means", "filtered_state_probs", "filtered_trans_probs", "forecasts"))
    dates, post, proper = hmc.altforecasts(d)
    cells = {s: hmc._read_csv(os.path.join(d, s + "_summary.csv")) for s in ("filtered_means", "filtered_state_probs", "filtered_trans_probs", "forecasts")}
    assert len(dates) == 460 == post.size == proper.size and dates == [r[0] for r in cells["forecasts"][1]]
    K = 3
    want, swapped = np.empty(460, dtype=LD), np.empty(460, dtype=LD)
    mumax = np.empty(460)
    for i in range(460):
        m, p, t = (np.array([float(x) for x in cells[s][1][i][1:]]).astype(LD) for s in ("filtered_means", "filtered_state_probs", "filtered_trans_probs"))
        Acm = t.reshape(K, K).T                                          # reshape(row, 3, 3) of Julia: A[i, j] = row[i + 3 j]
        w, ws = p.copy(), p.copy()
        for _ in range(12):
            w, ws = w @ Acm, ws @ Acm.T
        want[i], swapped[i], mumax[i] = w @ m, ws @ m, np.abs(m).max().astype(np.float64)
    bound = (2 * K * 12 + K) * 2.0 ** -52 * mumax
    diff = np.abs(post.astype(LD) - want).astype(np.float64)
    print("forecast_post: max |diff| = %.3e, bound there %.3e" % (diff.max(), bound[np.argmax(diff)]))
    assert (diff <= bound).all()
    col = cells["forecasts"][0].index("forecast_12_mean")
    assert [float(r[col]) for r in cells["forecasts"][1]] == list(proper)
    gap = np.abs(post - proper)
    worst = int(np.argmax(gap))
    print("largest |forecast_post - forecast_proper| = %.3f on %s" % (gap[worst], dates[worst]))
    assert gap[worst] > 0.1 and abs(gap[worst] - 0.281) < 1e-3
    # the transposed reshape gives another number there, far outside the bound
    assert abs(float(swapped[worst] - want[worst])) > 1e-3
    path = hmc.write_forecast_comparison(str(tmp_path / "forecast_comparision.csv"), dates, post, proper)
    header, rows = hmc._read_csv(path)
    assert header == ["date", "forecast_post", "forecast_proper"] and len(rows) == 460
    assert [r[0] for r in rows] == dates and [r[2] for r in rows] == [r[col] for r in cells["forecasts"][1]]
    assert [float(r[1]) for r in rows] == list(post) and [r[1] for r in rows] == [hmc._fmt(x) for x in post]


def _hand_made(seed, K=3, n=300):
    """Draws in the reference's Julia shapes: means, variances, states (n, K), A (n, K, K) with A[d, i, j]."""
    rng = np.random.default_rng(seed)
    means = np.sort(rng.normal(3.0, 2.5, size=(n, K)), axis=1)
    variances = 0.05 + rng.gamma(2.0, 0.8, size=(n, K))
    states = rng.dirichlet(np.ones(K), size=n)
    A = rng.dirichlet(np.ones(K) * 2.0, size=(n, K))
    return means, variances, states, A


def test_calcmoments_file_route_against_the_reference(tmp_path):
    """Per-draw files written by hmc.basicsave (through saveresults) from hand-made draws (K = 3, n = 300, two dates) through
    hmc.calcmoments (numpy, no GPU) against mixmoments_cases.reference on the same draws, rounded as the cells are."""
    dates = [dt.date(1980, 1, 1), dt.date(1985, 1, 1)]
    draws = [_hand_made(31 + i) for i in range(2)]
    for d, (means, variances, states, A) in zip(dates, draws):
        n, K = means.shape
        ds = [dt.date(1960 + i // 12, i % 12 + 1, 1) for i in range(11)] + [d]
        opt = hmc.estopt(np.zeros(12), ds, sampleRange=range(1, 13), endIndex=12, horizons=(12,), D=K, burnin=1, Nrun=n)
        s = hmc.Samples(means, variances, states[:, None, :], A, np.zeros((n, 2)), [d] * n)
        hmc.saveresults(s, opt, str(tmp_path), native=False)
    hz = (12, 0, 3)
    got_dates, got = hmc.calcmoments(str(tmp_path), dates, hz)
    assert got_dates == [str(d) for d in dates] and all(got[k].shape == (2, 3) for k in mc.FIELDS)
    for i, (means, variances, states, A) in enumerate(draws):
        abi = (means.T[None].copy(), variances.T[None].copy(), states.T[None].copy(), np.transpose(A, (2, 1, 0))[None].copy())
        ref = mc.reference(*abi, hz, True)
        mc.check({k: got[k][i:i + 1] for k in mc.FIELDS}, ref, mc.tolerance(ref, 300, 3, hz), "files %d" % i)
        assert all(np.isfinite(got[k][i]).all() for k in mc.FIELDS)
    _, h0 = hmc.calcmoments(str(tmp_path), dates[:1], (0,))
    assert all(np.array_equal(h0[k][0, 0], got[k][0, 1]) for k in mc.FIELDS)
    with pytest.raises(FileNotFoundError):
        hmc.calcmoments(str(tmp_path), [dt.date(1990, 1, 1)])


def test_batchresult_moments_is_none_unless_asked_for():
    res = hmc.BatchResult([], {"summary": np.zeros((0, 1)), "status": np.zeros(0, dtype=np.int32)}, False)
    assert res.moments is None
    with pytest.raises(ValueError, match="no mixture moments"):
        hmc.calcmoments("unused", ["1980-01-01"], result=res)
    res.moments = hmc.MixtureMoments((0,), {k: np.zeros((0, 1)) for k in _lib.MIX_FIELDS})
    with pytest.raises(ValueError, match="other horizons"):
        hmc.calcmoments("unused", [], (0, 12), result=res)
