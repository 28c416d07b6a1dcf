"""The width of the per-draw output block and the range of hmcg_config's scalar fields, on every kernel route.

The rest of the GPU suite varies T, K and the kernel form with H <= 3 horizons, blend_mask in {0, 1}, seeds below 2^32, window
ids below 2^31 and two prior settings.  The cases of tests/config_range_cases.py (held to their coverage contract without a
GPU by tests/test_config_range_cases.py) run H = 0..8 -- horizons 0, 1, 25 | 26 | 27, a repeated 12 and 5000 --, every
blend_mask bit with junk in the blended slots, 64-bit seeds, window ids with the top bit set and a window_base that wraps,
alpha = 3.5 / nu = 0.25, and one unknown (NaN) realised value per H = 8 row.  Per case:
  * oracle parity with the suite's own bar and checkers (states bit-exact, floats within TOL = 1e-9 relative to 1 + |x|,
    status the oracle's, a forecast cell NaN exactly where the oracle's is), and the timing record proves the route;
  * the forecasts against a reference that does not go through the oracle: pi_end[d]' A[d]^h mu[d] in numpy.longdouble from
    the call's own draws, same TOL (the oracle's own distance to that reference was measured at 1.6e-13, and is 2.4e-13 at
    most over the table as it stands; the CPU module bounds it by 1e-11; the kernels' is 1.9e-13 at most over the table).  Not on the tail path: there pi_end is the smoothed row at end_pos while the forecast
    starts from the last step.  The error column is the forecast minus yreal exactly; a repeated horizon repeats its column
    bit for bit;
  * summary / sample_summary against the mean of the 5-digit-rounded draws the call returned.
Then equalities between two GPU runs, all exact: the device entry, a chunked run (HMCG_CHUNK_DRAWS=2), three of four virtual
devices, window_base against the explicit wrapped ids, a chain cut with sweep_count / RESUME (every array, sumacc
included), extras.corr at H = 8 against H = 1; and a seed that differs in the high word only gives other draws."""
import numpy as np
import pytest

import config_range_cases as cr
import corr_cases as cc
import device_entry as de
from hmc_jl_amd import _lib
from device_entry import assert_device_equals_host, kept_after
from kernel_tables import FLAVOUR_WAVES, NT, REG_ROWS
from oracle_parity import (TOL, assert_same, check_against_oracle, check_signals_against_oracle, check_tail_signals_against_oracle, close,
                           close_nan)

pytestmark = pytest.mark.gpu
CASES = cr.CASES
IDS = [c.id for c in CASES]
H8 = [c for c in CASES if len(c.horizons) == 8]


def ids(cases):
    return [c.id for c in cases]


def set_env(monkeypatch, c):
    for k, v in c.env:
        monkeypatch.setenv(k, v)


_HOST = {}


def host_result(monkeypatch, c):
    """The case through the host entry, once per session; nothing changes it afterwards."""
    if c.id not in _HOST:
        set_env(monkeypatch, c)
        args, kw = cr.gpu_call(c)
        _HOST[c.id] = _lib.estimate_batch_host(*args, **kw)
    return _HOST[c.id]


def same_call(a, kw, c):
    """The call an oracle checker makes is the table's call of the case."""
    args, mine = cr.gpu_call(c)
    assert len(a) == len(args)
    for x, y in zip(a, args):
        assert (x is None and y is None) or np.array_equal(np.asarray(x), np.asarray(y), equal_nan=isinstance(x, np.ndarray) and x.dtype.kind == "f")
    on = {k: v for k, v in kw.items() if v is not None and v is not False}
    assert sorted(on) == sorted(mine), (sorted(on), sorted(mine))
    for k in on:
        assert np.array_equal(np.asarray(on[k]), np.asarray(mine[k])), k


def assert_route(g, c):
    """The timing record names the kernel the case is about."""
    planned, L = cr.planned_route(c)
    assert planned == c.route and g["steps_per_thread"] == L, (c.id, planned, g["steps_per_thread"], L)
    if c.route in ("register", "tpw"):
        assert g["occupancy"] in (1, 2) and not g["streaming"] and g["threads_per_window"] == (c.tpw or NT)
        flavour = dict(c.env).get("HMCG_FLAVOUR")
        if flavour:
            assert (g["helper_waves"], g["occupancy"]) == FLAVOUR_WAVES[flavour]
        assert any((k, l, nt) == (c.K, L, c.tpw or NT) for (k, l, nt, _, _, _, _) in REG_ROWS)
    else:
        assert g["occupancy"] == 0 and g["helper_waves"] == 0 and g["threads_per_window"] == NT
        assert g["streaming"] == (c.route == "stream")


# ---- oracle parity ----
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_case_against_oracle(hmclib, oracle, monkeypatch, c):
    def run(*a, **kw):
        same_call(a, kw, c)
        return host_result(monkeypatch, c)

    (Y, Tw, K, burnin, nrun, horizons, yreal), kw = cr.gpu_call(c)
    if c.path == "base":
        more = {k: kw[k] for k in ("window_base", "threads_per_window", "alpha", "nu") if k in kw}
        g = check_against_oracle(oracle, Y, Tw, K, burnin, nrun, horizons, yreal, window_ids=kw.get("window_ids"), seed=c.seed, run=run, **more)
    elif c.path == "sig":
        g = check_signals_against_oracle(oracle, Y, Tw, K, burnin, nrun, cr.N_SAMPLES, kw["sig_range"], kw["save_range"], cr.KAPPA, c.alpha,
                                         c.nu, kw["sigma_signal"], yreal, run=run, horizons=horizons, seed=c.seed, window_ids=kw.get("window_ids"))
    else:
        g = check_tail_signals_against_oracle(oracle, Y, Tw, K, burnin, nrun, cr.N_SAMPLES, kw["sig_range"], kw["save_range"], kw["sigma_signal"],
                                              kw["end_pos"], horizons, yreal, c.sigLen, want_sample_summary=True, run=run,
                                              blend_mask=cr.blend_mask(c), seed=c.seed, window_ids=kw.get("window_ids"))
    assert (g["status"] == 0).all()
    assert_route(g, c)
    H = len(horizons)
    assert g["fcast"].shape == (len(c.lens), 2 * H, g["mu"].shape[-1]) and g["summary"].shape == (len(c.lens), 3 * K + K * K + 2 * H)
    # unknown cells: the forecast columns never, an error column exactly where yreal is unknown; the same rows of the summaries
    unknown = np.repeat(np.isnan(yreal), 2, axis=1) & (np.arange(2 * H) % 2 == 1)
    assert np.array_equal(np.isnan(g["fcast"]), np.broadcast_to(unknown[:, :, None], g["fcast"].shape))
    assert np.array_equal(np.isnan(g["summary"]), np.concatenate([np.zeros((len(c.lens), 3 * K + K * K), bool), unknown], axis=1))


# ---- the forecasts from the call's own draws ----
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_forecasts_from_the_calls_own_draws(hmclib, monkeypatch, c):
    """Reference: pi_end[d]' A[d]^h mu[d] by square-and-multiply in numpy.longdouble from the returned draws (the labels are
    sorted in all three and the value is permutation-invariant).  Bar: TOL relative to 1 + |x|, the suite's; the oracle's own
    distance to this reference was measured at 1.6e-13 (2.4e-13 at most over this table, tests/test_config_range_cases.py)."""
    g = host_result(monkeypatch, c)
    (Y, Tw, K, burnin, nrun, horizons, yreal), kw = cr.gpu_call(c)
    fc = g["fcast"]
    for w in range(len(c.lens)):
        if c.path != "tail":
            d = cr.forecast_distance(fc[w].T, g["pi_end"][w].T, np.transpose(g["A"][w], (2, 1, 0)), g["mu"][w].T, horizons)
            print("%s window %d: forecast distance to the long-double reference %.3g" % (c.id, w, d))
            assert d < TOL, (c.id, w, d)
        for k in range(len(horizons)):
            assert np.array_equal(fc[w, 2 * k + 1], fc[w, 2 * k] - yreal[w, k], equal_nan=True), (c.id, w, k)
            assert np.isnan(fc[w, 2 * k + 1]).all() == bool(np.isnan(yreal[w, k])) and not np.isnan(fc[w, 2 * k]).any(), (c.id, w, k)
    twins = [(a, b) for a in range(len(horizons)) for b in range(a + 1, len(horizons))
             if horizons[a] == horizons[b] and (a in c.blend) == (b in c.blend)]
    assert twins or len(horizons) < 7 or c.blend, c.id
    for a, b in twins:
        assert np.array_equal(fc[:, 2 * a], fc[:, 2 * b]), (c.id, a, b)
    for a in c.blend:                          # every blended slot reports the same forecastsignal value
        assert np.array_equal(fc[:, 2 * a], fc[:, 2 * c.blend[0]]), (c.id, a)


# ---- the summaries from the call's own draws ----
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_summaries_from_the_calls_own_draws(hmclib, monkeypatch, c):
    """summary[w] = mean over all kept draws of round(x, 5), sample_summary[w, s] = the same over noise sample s; a NaN error
    column gives a NaN row."""
    g = host_result(monkeypatch, c)
    nrun = c.sweeps[1]
    for w in range(len(c.lens)):
        draws = [g[k][w] for k in ("mu", "sig2", "pi_end", "A", "fcast")]
        assert close_nan(g["summary"][w], cr.rounded_means(*draws)) < TOL, (c.id, w)
        if cr.is_sig(c):
            assert g["sample_summary"].shape[1] == cr.N_SAMPLES
            for s in range(cr.N_SAMPLES):
                part = [a[..., s * nrun:(s + 1) * nrun] for a in draws]
                assert close_nan(g["sample_summary"][w, s], cr.rounded_means(*part)) < TOL, (c.id, w, s)
        else:
            assert "sample_summary" not in g


# ---- equalities between two GPU runs (exact: oracle_parity.assert_same over every array) ----
DEVICE_CASES = [c for c in H8 if c.route in ("register", "lds")]


@pytest.mark.parametrize("c", DEVICE_CASES, ids=ids(DEVICE_CASES))
def test_device_entry_equals_host_entry(hmclib, monkeypatch, c):
    h = host_result(monkeypatch, c)
    set_env(monkeypatch, c)
    args, kw = cr.gpu_call(c)
    d = de.estimate_batch_device_np(*args, **kw)
    assert (d["status"] == 0).all()
    assert (d["steps_per_thread"], d["streaming"], d["occupancy"], d["helper_waves"]) == (h["steps_per_thread"], h["streaming"], h["occupancy"], h["helper_waves"])
    assert_device_equals_host(d, h, args[1], kw.get("save_range"))


@pytest.mark.parametrize("c", H8, ids=ids(H8))
def test_chunked_run_equals_one_launch(hmclib, monkeypatch, c):
    """Two kept draws per chunk: the 2H-wide forecast columns of every chunk land where the one-launch run put them."""
    one = host_result(monkeypatch, c)
    set_env(monkeypatch, c)
    monkeypatch.setenv("HMCG_CHUNK_DRAWS", "2")
    args, kw = cr.gpu_call(c)
    g = _lib.estimate_batch_host(*args, **kw)
    assert g["launches"] >= 2 and g["launches"] > one["launches"], (g["launches"], one["launches"])
    assert_same(g, one, what=c.id)


MULTI_CASES = [c for c in H8 if len(c.lens) >= 3]


@pytest.mark.parametrize("c", MULTI_CASES, ids=ids(MULTI_CASES))
def test_three_devices_equal_one(hmclib, monkeypatch, c):
    """hmcg_estimate_batch_multi over devices 0, 1, 2 of four virtual ones: every window keeps its id and its 2H-wide block."""
    one = host_result(monkeypatch, c)
    set_env(monkeypatch, c)
    monkeypatch.setenv("HMCG_VIRTUAL_DEVICES", "4")
    args, kw = cr.gpu_call(c)
    g = _lib.estimate_batch_host(*args, devices=[0, 1, 2], **kw)
    assert sorted(d["device"] for d in g["per_device"]) == [0, 1, 2] and sum(d["windows"] for d in g["per_device"]) == len(c.lens)
    assert all(d["windows"] > 0 for d in g["per_device"])
    assert_same(g, one, what=c.id)


WRAP_CASES = [c for c in CASES if c.window_base]


@pytest.mark.parametrize("c", WRAP_CASES, ids=ids(WRAP_CASES))
def test_wrapped_window_base_equals_explicit_ids(hmclib, monkeypatch, c):
    based = host_result(monkeypatch, c)
    set_env(monkeypatch, c)
    wrapped = np.array(cr.ids_of(c), dtype=np.uint32)
    assert wrapped.tolist() == [0xFFFFFFFE, 0xFFFFFFFF, 0]
    args, kw = cr.gpu_call(c, window_base=None, window_ids=wrapped)
    assert "window_base" not in kw
    assert_same(_lib.estimate_batch_host(*args, **kw), based, what=c.id)


SPLIT_CASES = [c for c in CASES if c.split]


@pytest.mark.parametrize("c", SPLIT_CASES, ids=ids(SPLIT_CASES))
def test_cut_chain_equals_one_launch(hmclib, monkeypatch, c):
    """sweep_count / HMCG_FLAG_RESUME on the device entry at H = 8: the pieces share one set of device buffers -- status, xstate,
    sumacc (NS + K wide, the pivots behind the 2H forecast sums), sample_summary -- and write their draws into the same arrays;
    every array equals the one-launch chain's, and that one the host entry's."""
    set_env(monkeypatch, c)
    args, kw = cr.gpu_call(c)
    burnin, nrun = c.sweeps
    n_samples = kw.get("n_samples", 1)
    total = n_samples * (burnin + nrun)
    one = de.estimate_batch_device_np(*args, **kw)
    assert (one["status"] == 0).all()
    assert_device_equals_host(one, host_result(monkeypatch, c), args[1], kw.get("save_range"))
    for cuts in cr.SPLIT_CUTS:
        g, base = None, 0
        for end in list(cuts) + [total]:
            g = de.estimate_batch_device_np(*args, **kw, sweep_base=base, sweep_count=end - base, resume_state=g)
            assert g["launches"] == 1 and (g["status"] == 0).all()
            d = kept_after(end, burnin, nrun, n_samples)
            for k in de.DRAW_KEYS:
                assert np.array_equal(g[k][..., :d], one[k][..., :d], equal_nan=True), (cuts, end, k)
                assert np.isnan(g[k][..., d:]).all(), (cuts, end, k, "a draw beyond this piece was written")
            base = end
        assert_same(g, one, what="%s cut after %s" % (c.id, cuts))


# ---- extras.corr ----
@pytest.mark.parametrize("cid", ["reg-K3-h-H8", "lds-K8-H8"])
def test_corr_does_not_depend_on_the_number_of_horizons(hmclib, monkeypatch, cid):
    """extras.corr reads the forecast of horizons[0] out of a 2H-wide block: the H = 8 run's matrix equals the H = 1 run's bit
    for bit, and the Pearson matrix of the rounded draws in long double within min(the bound derived in corr_cases, 1e-10), as in
    test_gpu_corr.py."""
    c = cr.BY_ID[cid]
    set_env(monkeypatch, c)
    args8, kw8 = cr.gpu_call(c, sweeps=cr.CORR_SWEEPS, want_corr=True)
    args1, kw1 = cr.gpu_call(c, sweeps=cr.CORR_SWEEPS, want_corr=True, horizons=c.horizons[:1])
    g8, g1 = _lib.estimate_batch_host(*args8, **kw8), _lib.estimate_batch_host(*args1, **kw1)
    assert (g8["status"] == 0).all() and g8["fcast"].shape[1] == 16 and g1["fcast"].shape[1] == 2
    assert np.array_equal(g8["corr"], g1["corr"], equal_nan=True)
    K = c.K
    for w, T in enumerate(c.lens):
        cols = np.concatenate([g8["mu"][w], g8["sig2"][w], g8["pi_end"][w], g8["A"][w].reshape(K * K, -1), g8["fcast"][w, :1]], axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            ref = np.corrcoef(np.round(cols, 5).astype(np.longdouble))
        got = g8["corr"][w]
        ok = np.isfinite(ref)
        assert np.array_equal(np.isfinite(got), ok), (cid, w)
        assert T < 10 or ok.all(), (cid, w)                    # (a two-step window's draws may be constant after rounding)
        assert not ok.any() or float(np.abs(got[ok] - ref[ok]).max()) < 1e-10, (cid, w)
        # ... and within min(the derived bound, 1e-10) of corr_cases' reference (moments about the first draw, long double)
        cc.check(got[None], cc.reference(cols[None], cols.shape[-1]), "%s window %d" % (cid, w), cap=1e-10)


# ---- the seed's high word ----
@pytest.mark.parametrize("cid", ["reg-K3-p1-H6", "lds-K7-H7"])
def test_seed_high_word_reaches_the_generator(hmclib, oracle, monkeypatch, cid):
    """seed = 1234 + 2^32 and seed = 1234 share the low key word of Philox: other draws, each run matching its own oracle run."""
    c = cr.BY_ID[cid]
    assert c.seed == cr.SEED_HIGH_WORD and c.path == "base"
    high = host_result(monkeypatch, c)
    set_env(monkeypatch, c)
    (Y, Tw, K, burnin, nrun, horizons, yreal), kw = cr.gpu_call(c)
    low = check_against_oracle(oracle, Y, Tw, K, burnin, nrun, horizons, yreal, seed=cr.SEED_DEFAULT)
    for w in range(len(c.lens)):
        assert not np.array_equal(low["mu"][w], high["mu"][w]), (cid, w)
        assert close(low["mu"][w], high["mu"][w]) > TOL, (cid, w)
