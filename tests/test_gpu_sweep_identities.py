"""One sweep's filter, smoother, reported row and forecasts on every smoothing-capable kernel form, against the reference's
formulas in numpy.longdouble (tests/sweep_identities.py) -- no oracle in between -- and, new on the GPU, end_pos together with the
smoothing outputs: the ten <K, L, 256, SIG = 1, SM = 1> register rows' classes, g_big_110 and the streaming SIG + SM form with
signals past the end date, where the kernels build pi_end by a backward vector product of their own (gibbs_device.hpp, the
outputs job; gibbs_big.hpp, OUT_WAVE) beside the full smoother.

Per case of sweep_identities.CASES (nrun = 1, n_samples = 1; the same table tests/test_sweep_identities.py runs on the oracle):
  * the timing record proves which kernel ran (row and flavour / LDS-resident / streaming);
  * the four residuals <= TOL = 1e-9, the suite's tolerance for every float the kernels produce; pi_smooth_draws[..., 0] is
    pi_smooth_mean bit for bit (a mean of one draw);
  * two routes, one row: pi_end against the call's own pi_smooth_mean[end_pos] within TOL (two different recursions on the
    device: no bit equality asked);
  * the usual contract against the oracle: status, x_final exact, every float output within TOL.
Then per form (register, LDS-resident, streaming) one tail-with-smoothing call of 3 noise samples x 4 kept draws against the oracle
(sample parity selects the staged last observation), and two of the cases through the device entry over sentinel-prefilled
buffers: bit-identical to the host entry, nothing written beyond T[w].

Largest residuals seen on the MI355X per family (the oracle's own over the same table: filter 1.0e-15, smoother 2.5e-14, row
4.1e-15, forecasts 5.7e-16):
                            filter    smoother  reported row  forecasts  two routes
    register SM             2.1e-15   2.0e-13   0             2.5e-16    1.4e-15
    LDS-resident SM         2.5e-15   2.2e-13   0             3.8e-16    1.4e-15
    streaming SM            1.9e-15   1.0e-12   0             1.1e-16    1.2e-15
    register SIG + SM       1.8e-15   5.5e-14   0             1.4e-16    2.2e-16
    LDS-resident SIG + SM   1.2e-15   3.0e-14   0             2.3e-16    2.2e-16
    register tail + SM      1.9e-15   1.9e-13   2.8e-14       1.8e-16    1.1e-16
    LDS-resident tail + SM  1.9e-15   2.0e-13   2.8e-14       5.7e-16    2.2e-16
    streaming tail + SM     1.9e-15   6.7e-13   2.1e-14       2.4e-16    1.1e-16
The smoother's 1e-12 at T = 7935 is the scan's error over the longest window, three decades inside TOL; the smallest filtered
probability was 9.0e-176 and no step of any of the 109 windows was left out.  No kernel fault or wrong number showed."""
import numpy as np
import pytest

import device_entry as de
import sweep_identities as si
from hmc_jl_amd import _lib
from device_entry import assert_device_equals_host
from kernel_tables import FLAVOUR_WAVES, NT, ladder_ceiling
from oracle_parity import TOL, assert_ran_on_big, assert_window_matches_oracle

pytestmark = pytest.mark.gpu


def assert_ran_as_planned(g, c, kw):
    sig, top = "sig_range" in kw, max(c["lens"])
    if c["kernel"] == "register":
        assert top <= ladder_ceiling(c["K"], sig, True), c["id"]
        assert g["threads_per_window"] == NT and g["steps_per_thread"] == c["L"], (g["threads_per_window"], g["steps_per_thread"], c["L"])
        assert g["buckets"] == 1 and not g["streaming"]
        # the SIG + SM rows are compiled in the plain flavour alone
        assert (g["helper_waves"], g["occupancy"]) == (FLAVOUR_WAVES[c["flavour"]] if c["flavour"] else (0, 1)), (g["helper_waves"], g["occupancy"])
    else:
        assert top > ladder_ceiling(c["K"], sig, True), c["id"]            # the production route, no HMCG_FORCE_BIG
        assert_ran_on_big(g, c["kernel"] == "stream", top, sig, True)


def check_window_against_oracle(g, args, kw, w, o):
    """The suite's contract for window w: status equal, states exact, every float within TOL."""
    fields = ("mu", "sig2", "A", "pi_end", "pif_final", "pi_smooth_mean", "pi_filter_mean", "pi_smooth_draws")
    n = int(kw["sig_range"][w][1] - kw["sig_range"][w][0]) if "sig_range" in kw else None
    assert_window_matches_oracle(g, w, int(args[1][w]), o, fields=fields + (("sigvals",) if n is not None else ()),
                                 nan_fields=("fcast", "summary"), nsave=n)


@pytest.mark.parametrize("c", si.CASES, ids=si.CASE_IDS)
def test_one_sweep_against_the_formulas(hmclib, oracle, monkeypatch, c):
    if c["flavour"]:
        monkeypatch.setenv("HMCG_FLAVOUR", c["flavour"])
    args, kw, runs = si.oracle_runs(oracle, c)
    g = _lib.estimate_batch_host(*args, **kw)
    assert_ran_as_planned(g, c, kw)
    failed = []
    for w, T in enumerate(c["lens"]):
        assert g["status"][w] == 0, (w, g["status"][w])
        assert np.array_equal(g["pi_smooth_draws"][w, :, :T, 0].T, g["pi_smooth_mean"][w, :T]), w
        pos, wkw = si.library_inputs(args, kw, w, g)
        r = si.residuals(*pos, **wkw)
        rep = wkw.get("end_pos", T - 1)
        routes = float(np.max(np.abs(g["pi_end"][w, :, 0] - g["pi_smooth_mean"][w, rep])))
        what = "%s window %d (T = %d): %s, two routes %.2e" % (c["id"], w, T, si.describe(r), routes)
        print(what)
        if not (r["min_pif"] > 0 and r["left_out"] == 0 and all(r[k] <= TOL for k in si.IDENTITIES) and routes <= TOL):
            failed.append(what)
    assert not failed, "\n".join(failed)
    for w, o in enumerate(runs):
        check_window_against_oracle(g, args, kw, w, o)


@pytest.mark.parametrize("id", si.MULTI_SAMPLE)
def test_tail_with_smoothing_over_noise_samples(hmclib, oracle, id):
    c = si.case_by_id(id)
    assert c["path"] == "tail+smooth"
    args, kw = si.call_of(c, n_samples=3, nrun=4)
    g = _lib.estimate_batch_host(*args, **kw)
    assert_ran_as_planned(g, c, kw)
    for w in range(len(c["lens"])):
        check_window_against_oracle(g, args, kw, w, si.oracle_window(oracle, args, kw, w, n_samples=3))
        rep = int(kw["end_pos"][w])
        assert np.max(np.abs(g["pi_end"][w] - g["pi_smooth_draws"][w, :, rep, :])) <= TOL, w


@pytest.mark.parametrize("id", si.DEVICE_ENTRY)
def test_tail_with_smoothing_through_the_device_entry(hmclib, id):
    c = si.case_by_id(id)
    assert c["path"] == "tail+smooth"
    args, kw = si.call_of(c)
    d = de.estimate_batch_device_np(*args, **kw)
    assert (d["status"] == 0).all(), d["status"]
    assert_ran_as_planned(d, c, kw)
    h = _lib.estimate_batch_host(*args, **kw)
    assert (h["steps_per_thread"], h["streaming"], h["occupancy"]) == (d["steps_per_thread"], d["streaming"], d["occupancy"])
    assert_device_equals_host(d, h, args[1], kw["save_range"])
