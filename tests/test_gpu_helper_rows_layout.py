"""The six-barrier helper rows with X[T-1] drawn by a helper wave -- gibbs<2,4,256,0,0,4,2>, gibbs<3,4,256,0,0,4,2> and
gibbs<2,4,256,0,1,4,2> (gibbs_device.hpp, HELPER_DRAW) -- held to the plain flavour of the same row and to the oracle.  The
module exists for changes that touch only where those rows' code lies (block placement, cold paths moved behind the sweep
loops, one copy of a twin loop): such a change must leave every output bit as it was, and the plain flavour (HMCG_FLAVOUR=p1,
no helper waves, another kernel instantiation) is the in-suite witness of "as it was".

Cases: each row at T in LENGTHS -- the owner of step T-1 in the first lane of wave 3 (769, 770), mid-wave (1000) and in the
block's last thread (1021, 1024), with 0 to 3 padded slots in the owner's chunk -- three windows of that length, no burn-in and
six kept sweeps, as one launch and as two resumed launches of three.  Per case:

  * mu, sig2, A, pi_end, fcast, summary and status array_equal between HMCG_FLAVOUR=h and HMCG_FLAVOUR=p1 (x_final and, in the
    smoothing row, pi_smooth_mean too);
  * the same seven array_equal between the single launch and the two resumed ones;
  * against the oracle with oracle_parity's bar: states exact, floats within TOL = 1e-9;
  * the launch report (the library's hmcg_timing, as DevicePanel.last_timing holds it) names the row: four steps per thread on
    256 threads, four helper waves in the helper flavour and none in the plain one.

COLD is one more case: K = 3, T = 1000, the window id at which the oracle's branch counters show a gamma draw of the A rows
that needs a third Marsaglia-Tsang attempt within the six sweeps (searched on the CPU oracle, ids 0..2999 of this data: 1712 is
the only one) -- the inline-Philox path of attempts >= 3, which a layout change moves out of the sweep loop, then executes.
The test at the end of the file, which needs no GPU, holds the case table to these claims."""
import numpy as np
import pytest

import kernel_tables as kt
from hmc_jl_amd import _lib, synth
from oracle_parity import assert_same, assert_window_matches_oracle, forced_flavour_call

gpu = pytest.mark.gpu
L, NT = 4, kt.NT
W, NRUN, CUT, HORIZONS = 3, 6, 3, (1, 12)
OUTPUTS = ("mu", "sig2", "A", "pi_end", "fcast", "summary", "status")
FLOATS = OUTPUTS[:-1]
ROWS = {"K3-base": (3, False), "K2-base": (2, False), "K2-smooth": (2, True)}       # row -> (K, smoothing)
LENGTHS = (769, 770, 1000, 1021, 1024)
CASES = [(row, T) for row in ROWS for T in LENGTHS]
COLD_K, COLD_T, COLD_ID = 3, 1000, 1712


def owner(T):
    """(wave, lane, padded slots in the owner's chunk) of step T-1."""
    tid, slot = divmod(T - 1, L)
    return tid // 64, tid % 64, L - 1 - slot


def ran_on(g, flavour):
    assert g["steps_per_thread"] == L and g["threads_per_window"] == NT and g["buckets"] == 1
    assert (g["helper_waves"], g["occupancy"]) == kt.FLAVOUR_WAVES[flavour], (flavour, g["helper_waves"], g["occupancy"])


def hold_to_oracle_and_plain(monkeypatch, args, kw, K, smooth, refs):
    """One call's three runs -- helper flavour in one launch, helper flavour in two resumed launches, plain flavour -- against
    each other and the oracle's runs `refs` of the windows."""
    monkeypatch.setenv("HMCG_NO_BUCKETS", "1")
    more = dict(want_smooth=True) if smooth else {}
    h = forced_flavour_call(monkeypatch, "h", *args, **kw, **more)
    p = forced_flavour_call(monkeypatch, "p1", *args, **kw, **more)
    a = forced_flavour_call(monkeypatch, "h", *args, sweep_count=CUT, **kw, **more)
    b = forced_flavour_call(monkeypatch, "h", *args, resume_state=a, sweep_base=CUT, **kw, **more)
    for g, fl in ((h, "h"), (a, "h"), (b, "h"), (p, "p1")):
        ran_on(g, fl)
    assert_same(h, p, OUTPUTS + ("x_final",) + (("pi_smooth_mean",) if smooth else ()), equal_nan=False, what="h against p1")
    for k in ("mu", "sig2", "pi_end", "fcast", "A"):                 # the draw index is the last axis
        assert np.array_equal(a[k][..., :CUT], h[k][..., :CUT]), ("first launch", k)
        assert np.array_equal(b[k][..., CUT:], h[k][..., CUT:]), ("resumed launch", k)
    assert_same(b, h, ("summary", "status", "x_final"), equal_nan=False, what="resumed against single")
    fields = FLOATS + (("pi_smooth_mean",) if smooth else ())
    for w, o in enumerate(refs):
        assert_window_matches_oracle(h, w, int(args[1][w]), o, fields=fields)


_refs = {}


def panel(K, T):
    Y, Tw, fut = synth.generate_panel(W, T, K)
    return Y, Tw, np.ascontiguousarray(fut[:, [0, 11]]), np.arange(40, 40 + W)


def reference(oracle, K, T, smooth):
    """The oracle's runs of a (K, T) panel, once: the smoothing row reads the run that also has the smoothed means."""
    if (K, T, smooth) not in _refs:
        Y, Tw, yreal, ids = panel(K, T)
        _refs[K, T, smooth] = [oracle.estimate_window(Y[w, :T], K, 0, NRUN, HORIZONS, yreal[w], window_id=int(ids[w]), want_smooth=smooth)
                               for w in range(W)]
    return _refs[K, T, smooth]


@gpu
@pytest.mark.parametrize("row,T", CASES, ids=["%s-T%d" % c for c in CASES])
def test_helper_row_equals_plain_row_and_oracle(hmclib, oracle, monkeypatch, row, T):
    K, smooth = ROWS[row]
    Y, Tw, yreal, ids = panel(K, T)
    hold_to_oracle_and_plain(monkeypatch, (Y, Tw, K, 0, NRUN, HORIZONS, yreal), dict(window_ids=ids), K, smooth,
                             reference(oracle, K, T, smooth))


def cold_inputs():
    Y, Tw, fut = synth.generate_panel(1, COLD_T, COLD_K)
    return Y, Tw, np.ascontiguousarray(fut[:, [0, 11]]), np.array([COLD_ID])


def cold_reference(oracle):
    Y, Tw, yreal, ids = cold_inputs()
    return oracle.estimate_window(Y[0], COLD_K, 0, NRUN, HORIZONS, yreal[0], window_id=COLD_ID)


@gpu
def test_third_gamma_attempt_runs_in_the_helper_row(hmclib, oracle, monkeypatch):
    Y, Tw, yreal, ids = cold_inputs()
    o = cold_reference(oracle)
    assert o["branches"]["gamma_3plus"] >= 1
    hold_to_oracle_and_plain(monkeypatch, (Y, Tw, COLD_K, 0, NRUN, HORIZONS, yreal), dict(window_ids=ids), COLD_K, False, [o])


# ---- the contract of the tables above: no GPU ----
def test_case_table_covers_what_it_claims(oracle):
    for K, smooth in ROWS.values():
        assert (K, L, "smooth" if smooth else "base") in kt.VARIANT_ROWS
        assert all(kt.steps_per_thread(K, T, False, smooth) == L for T in LENGTHS)
    assert kt.FLAVOUR_WAVES["h"][0] == 4 and kt.FLAVOUR_WAVES["p1"][0] == 0
    assert owner(769) == (3, 0, 3) and owner(770) == (3, 0, 2)              # wave 3's first lane
    assert owner(1000) == (3, 57, 0)                                       # mid-wave
    assert owner(1021) == (3, 63, 3) and owner(1024) == (3, 63, 0)          # the block's last thread
    assert {owner(T)[2] for T in LENGTHS} == {0, 2, 3} and 0 < CUT < NRUN and W == 3
    br = cold_reference(oracle)["branches"]
    assert br["gamma_3plus"] >= 1 and br["gamma_3plus_A"] + br["gamma_3plus_sig2"] == br["gamma_3plus"], br
    assert kt.steps_per_thread(COLD_K, COLD_T) == L
