"""How a result of the library is held against the oracle on the same seeded inputs.  A plain module for the GPU tests;
nothing here is collected.

Bar: state paths (integers) bit-exact; floating-point draws, filtered probabilities and summaries within TOL = 1e-9
relative-to-(1+|x|) -- BASELINE.json's north_star tolerance ("filtered state probabilities within 1e-9 of reference"); observed
~1e-14.  The GPU path is a time-parallel scan, the oracle is sequential, so bitwise float equality is not expected; a
categorical draw can only flip when a uniform lands within ~1e-14 of a CDF boundary, which the suite's fixed seeds do not do.

assert_window_matches_oracle is the one per-window comparison: it owns the views that turn the C-ABI layouts of a call's result
into the oracle's (draw index first, steps cut at T).  The check_* functions run a call (run=: the entry under test with
estimate_batch_host's interface; tests/device_entry.py has the device entry's) and the oracle window by window, and compare
through it.  assert_same is the comparison between two runs of the library: exact.  tests/test_oracle_parity_helpers.py pins,
without a GPU, that each of them fails when it should."""
import numpy as np

from hmc_jl_amd import _lib
from kernel_tables import LDS_LIMIT, NT, dyn_bytes

TOL = 1e-9
FLOAT_KEYS = ("mu", "sig2", "A", "pi_end", "fcast", "summary", "pif_final")
DRAWS_FIRST = ("mu", "sig2", "pi_end", "fcast")                                      # (K | 2H, nd) -> the oracle's (nd, K | 2H)
CUT_AT_T = ("x_final", "pif_final", "pi_smooth_mean", "pi_filter_mean")              # (ldY, ...) -> the window's own T steps
ORACLE_NAME = {"pi_smooth_draws": "pi_smooth"}                                       # samples.pib itself: (nd, T, K)


def close(g, o, tol=TOL):
    return float(np.max(np.abs(g - o) / (1.0 + np.abs(o)))) if g.size else 0.0


def close_nan(g, o):
    """close() over arrays whose cells may be NaN (a forecast error whose realised value is unknown, its summary rows): inf
    unless both are NaN in the same cells, else close() of the others.  Without a NaN it is close()."""
    g, o = np.asarray(g), np.asarray(o)
    unknown = np.isnan(o)
    if not np.array_equal(np.isnan(g), unknown):
        return float("inf")
    return close(g[~unknown], o[~unknown])


def window_view(g, w, T, k, nsave=None):
    """Field k of window w of a result in the oracle's layout."""
    a = g[k][w]
    if k in DRAWS_FIRST:
        return a.T
    if k == "A":
        return np.transpose(a, (2, 1, 0))
    if k in CUT_AT_T:
        return a[:T]
    if k == "pi_smooth_draws":
        return np.transpose(a[:, :T, :], (2, 1, 0))
    if k == "sigvals":
        return a[:, :nsave]
    return a


def oracle_field(o, k):
    return o["pi_smooth"].mean(axis=0) if k == "pi_smooth_mean" else o[ORACLE_NAME.get(k, k)]


def assert_window_matches_oracle(g, w, T, o, fields=FLOAT_KEYS, nan_fields=(), known_fields=(), nsave=None, status0=True, states=True):
    """Window w (T steps) of the result g against the oracle's run o of that window: status equal (status0: and 0), x_final
    bit-exact over the window's steps (states=False: the entry returns none), every field of `fields` within TOL through
    close(), of `nan_fields` through close_nan() (NaN exactly where the oracle's is), of `known_fields` through close() over the
    cells the oracle knows (not NaN).  nsave: the saved positions of `sigvals`, where that is asked for."""
    assert g["status"][w] == o["status"], "window %d: status %s, the oracle's %s" % (w, g["status"][w], o["status"])
    assert not status0 or o["status"] == 0, "window %d: status %s" % (w, o["status"])
    if states:
        assert np.array_equal(g["x_final"][w, :T], o["x_final"]), "window %d: x_final, the state path, differs from the oracle's" % w
    for k in tuple(fields) + tuple(nan_fields) + tuple(known_fields):
        got, want = np.asarray(window_view(g, w, T, k, nsave)), np.asarray(oracle_field(o, k))
        assert got.shape == want.shape, "window %d: %s has shape %s, the oracle's %s" % (w, k, got.shape, want.shape)
        if k in nan_fields:
            err = close_nan(got, want)
        elif k in known_fields:
            known = ~np.isnan(want)
            err = close(got[known], want[known])
        else:
            err = close(got, want)
        assert err < TOL, "window %d: %s differs from the oracle by %.3g (relative to 1 + |x|; TOL %g)" % (w, k, err, TOL)


def assert_batch_matches_oracle(g, o, fields):
    """A whole result against oracle.estimate_batch's (the same layouts): status 0, states exact, `fields` within TOL."""
    assert (g["status"] == 0).all(), g["status"]
    assert np.array_equal(g["x_final"], o["x_final"]), "state paths differ"
    for k in fields:
        err = close(g[k], o[k])
        print(k, err)
        assert err < TOL, (k, err)


def assert_same(a, b, keys=None, equal_nan=True, what=""):
    """Two runs of the library, bit for bit: the arrays of `keys` (None: every array of either, and both hold the same ones);
    NaN equals NaN in float arrays unless equal_nan=False."""
    if keys is None:
        A, B = ({k for k, v in r.items() if isinstance(v, np.ndarray)} for r in (a, b))
        assert A == B, (what, sorted(A ^ B))
        keys = sorted(A)
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert np.array_equal(x, y, equal_nan=equal_nan and x.dtype.kind == "f"), (what, k)


def forced_flavour_call(monkeypatch, flavour, *args, **kw):
    """_lib.estimate_batch_host(*args, want_state=True, **kw) under HMCG_FLAVOUR = flavour (None: the table's own choice)."""
    if flavour is None:
        monkeypatch.delenv("HMCG_FLAVOUR", raising=False)
    else:
        monkeypatch.setenv("HMCG_FLAVOUR", flavour)
    g = _lib.estimate_batch_host(*args, want_state=True, **kw)
    if flavour is not None:
        assert g["helper_waves"] == (4 if flavour == "h" else 0)
    return g


# ---- what proves that the intended instantiation ran ----
def assert_ran_on_big(g, stream, maxT, sig=False, smooth=False):
    L = (maxT + NT - 1) // NT
    assert g["occupancy"] == 0, g["occupancy"]                       # the OCC template argument: 0 = the LDS-resident kernel
    assert g["helper_waves"] == 0 and g["buckets"] == 1
    assert g["threads_per_window"] == NT and g["steps_per_thread"] == L, (g["threads_per_window"], g["steps_per_thread"], L)
    assert g["streaming"] == stream
    if stream:
        assert 16 <= g["lds_bytes"] < dyn_bytes(L)                   # its per-step arrays are in HBM
    else:
        assert dyn_bytes(L) <= g["lds_bytes"] <= LDS_LIMIT
    assert ("sigvals" in g) == sig and ("pi_smooth_mean" in g) == smooth     # make_plan takes the path from the extras passed


# ---- a call and the oracle, window by window ----
def check_against_oracle(oracle, Y, Tw, K, burnin, nrun, horizons=(12,), yreal=None, window_ids=None, seed=1234,
                         run=_lib.estimate_batch_host, **kw):
    g = run(Y, Tw, K, burnin, nrun, horizons, yreal, seed=seed, want_state=True, window_ids=window_ids, **kw)
    W = Y.shape[0]
    alpha, nu = kw.get("alpha") or 1.0, kw.get("nu") or 1.0
    for w in range(W):
        wid = (kw.get("window_base", 0) + w) & 0xFFFFFFFF if window_ids is None else int(window_ids[w])
        yr = None if yreal is None else yreal[w]
        if (alpha, nu) == (1.0, 1.0):
            o = oracle.estimate_window(Y[w, :Tw[w]], K, burnin, nrun, horizons, yr, seed=seed, window_id=wid)
        else:                                  # the base-path run at other priors: estimate_signals with an empty signal set
            o = oracle.estimate_signals(Y[w, :Tw[w]], K, burnin, nrun, 1, alpha=alpha, nu=nu, horizons=horizons, yreal=yr,
                                        seed=seed, window_id=wid)
        # without yreal the error columns are not held to the oracle's; the forecast columns always are
        assert_window_matches_oracle(g, w, Tw[w], o, fields=("mu", "sig2", "A", "pi_end", "pif_final"), known_fields=("summary",),
                                     nan_fields=("fcast",) if len(horizons) and yreal is not None else (), status0=False)
        if len(horizons):
            assert close(g["fcast"][w, 0::2].T, o["fcast"][:, 0::2]) < TOL, "window %d: fcast (the forecast columns)" % w
    return g


def check_signals_against_oracle(oracle, Y, Tw, K, burnin, nrun, n_samples, sig, save, kappa, alpha, nu, ssig, yreal,
                                 run=_lib.estimate_batch_host, horizons=(12,), seed=1234, window_ids=None):
    W = Y.shape[0]
    g = run(Y, Tw, K, burnin, nrun, horizons, yreal, want_state=True, sig_range=sig, save_range=save, seed=seed, window_ids=window_ids,
            sigma_signal=ssig, kappa=kappa, n_samples=n_samples, alpha=alpha, nu=nu, want_sample_summary=True)
    for w in range(W):
        o = oracle.estimate_signals(Y[w, :Tw[w]], K, burnin, nrun, n_samples, sig=tuple(sig[w]), kappa=kappa, alpha=alpha,
                                    nu=nu, sigma_signal=float(ssig[w]), save=tuple(save[w]), horizons=horizons, yreal=yreal[w],
                                    seed=seed, window_id=w if window_ids is None else int(window_ids[w]))
        assert_window_matches_oracle(g, w, Tw[w], o, fields=("mu", "sig2", "A", "pi_end", "sigvals", "pif_final"),
                                     nan_fields=("fcast", "summary", "sample_summary"),       # sample_summary: runaggregate's (date, signalid) rows
                                     nsave=save[w][1] - save[w][0])
    return g


def check_tail_signals_against_oracle(oracle, Y, Tw, K, burnin, nrun, n_samples, sig, save, ssig, end_pos, horizons, yreal, sigLen,
                                      want_sample_summary=False, run=_lib.estimate_batch_host, blend_mask=1, seed=1234, window_ids=None):
    """Signals past the end date (end_pos, blend_mask: the horizon slots that equal sigLen; kappa = 0.6, alpha = nu = 2) against
    the oracle, window by window."""
    more = dict(want_sample_summary=True) if want_sample_summary else {}
    g = run(Y, Tw, K, burnin, nrun, horizons, yreal, want_state=True, sig_range=sig, save_range=save, seed=seed, window_ids=window_ids,
            sigma_signal=ssig, kappa=0.6, n_samples=n_samples, alpha=2.0, nu=2.0, end_pos=end_pos, blend_mask=blend_mask, **more)
    for w in range(Y.shape[0]):
        o = oracle.estimate_signals(Y[w, :Tw[w]], K, burnin, nrun, n_samples, sig=tuple(sig[w]), kappa=0.6, alpha=2.0, nu=2.0,
                                    sigma_signal=float(ssig[w]), save=tuple(save[w]), horizons=horizons, yreal=yreal[w], seed=seed,
                                    window_id=w if window_ids is None else int(window_ids[w]), end_pos=int(end_pos[w]),
                                    blend_mask=blend_mask)
        assert_window_matches_oracle(g, w, Tw[w], o, fields=("mu", "sig2", "pi_end", "sigvals"),
                                     nan_fields=("fcast", "summary") + (("sample_summary",) if want_sample_summary else ()), nsave=sigLen)
        assert np.max(np.abs(g["pi_end"][w].sum(axis=0) - 1)) < 1e-12
    return g


def check_teacher_forced_against_oracle(oracle, Y, Tw, K, x_init, run=_lib.estimate_batch_host):
    """One sweep from given states (full-length windows): the redrawn states exact, the filtered-probability path and the
    parameter draws within TOL."""
    g = run(Y, Tw, K, 0, 1, (), None, x_init=x_init, want_state=True)
    for w in range(Y.shape[0]):
        o = oracle.estimate_window(Y[w], K, 0, 1, (), None, window_id=w, x_init=x_init[w])
        assert_window_matches_oracle(g, w, Y.shape[1], o, fields=("pif_final", "mu", "A"), status0=False)
    return g


# the signal ranges of the LDS-resident coverage cases (tests/test_gpu_big_variants.py) and of the device-entry cases built on them
SIG_LEN = (40, 1, None, 12, 40)                                   # per window: a tail, one step, everything a signal, tails
SAVE_LEN = (3, 1, 2, 3, 2)
SIGMA_SIGNAL = np.array([0.5, 1.0, 0.2, 0.8, 0.3])


def signal_ranges(Tw):
    sig = np.array([[T - (T if n is None else n), T] for T, n in zip(Tw, SIG_LEN)], dtype=np.int32)
    save = np.array([[T - n, T] for T, n in zip(Tw, SAVE_LEN)], dtype=np.int32)
    return sig, save


def check_smoothing_against_oracle(oracle, Y, Tw, K, burnin, nrun, yreal, sig=None, ssig=None, n_samples=1,
                                   run=_lib.estimate_batch_host, **more):
    """extras.pi_smooth_mean / pi_filter_mean against the mean of the oracle's literal Pb recursion and its running filtered
    mean, with every other output; sig: on the signal path (as test_smoothed_means_on_the_signal_path_lds_resident_kernel)."""
    kw = dict(sig_range=sig, save_range=sig, sigma_signal=ssig, kappa=0.6, n_samples=n_samples, alpha=2.0, nu=2.0) if sig is not None else {}
    g = run(Y, Tw, K, burnin, nrun, (12,), yreal, want_state=True, want_smooth=True, want_filter_mean=True, **kw, **more)
    fields = FLOAT_KEYS + ("pi_smooth_mean", "pi_filter_mean")
    if "pi_smooth_draws" in g:                                   # asked for through `more`: samples.pib[Nrun, N, D] itself
        fields += ("pi_smooth_draws",)
    for w in range(Y.shape[0]):
        T = int(Tw[w])
        if sig is not None:
            o = oracle.estimate_signals(Y[w, :T], K, burnin, nrun, n_samples, sig=tuple(sig[w]), kappa=0.6, alpha=2.0, nu=2.0,
                                        sigma_signal=float(ssig[w]), save=tuple(sig[w]), yreal=yreal[w], window_id=w,
                                        want_smooth=True, want_filter_mean=True)
            assert_window_matches_oracle(g, w, T, o, fields=fields + ("sigvals",), nsave=sig[w][1] - sig[w][0])
        else:
            o = oracle.estimate_window(Y[w, :T], K, burnin, nrun, (12,), yreal[w], window_id=w, want_smooth=True)
            o["pi_filter_mean"] = oracle.estimate_signals(Y[w, :T], K, burnin, nrun, 1, horizons=(12,), yreal=yreal[w], window_id=w,
                                                          want_filter_mean=True)["pi_filter_mean"]
            assert_window_matches_oracle(g, w, T, o, fields=fields)
        assert np.max(np.abs(g["pi_smooth_mean"][w, :T].sum(axis=1) - 1)) < 1e-12
    return g
