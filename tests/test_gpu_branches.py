"""Label permutation and the rare draw branches, in every kernel form, against the oracle.

The per-instantiation tests (test_gpu_variants.py, test_gpu_big_variants.py) prove that every compiled kernel is RUN against
the oracle; their data (synth.generate_panel: regimes three and more standard deviations apart, argmax start, alpha 1 or 2)
keep the chain on one side of every data-dependent branch.  The oracle's branch counters (oracle/hmc_oracle.c, BC_*;
out["branches"]) on the case lists as they stood before this module -- oracle alone, on the CPU:

                                     per-variant   sigsmooth   LDS-resident:    its longest    fuzz, 96    k8 edges
                                     (39 x 2 win)  (10 x 2)    56 x 5 windows   window alone   base cases
    sweeps                                 700        360          1960             392          1211         18
    ... sortperm(mu) not the identity       15         12          1022              20           236         12
    ... not its own inverse                  0          0           706               0           143          7
    gamma draws, first attempt            8618       4399         37232           12116         30098        698
    ... second attempt                      10         13           334              40           188          5
    ... third or later: SIG2 / A           0 / 1      0 / 0        0 / 8           0 / 0         0 / 3       0 / 1
    v <= 0 rejections                        0          0             0               0             0          0
    shape == 1 / shape < 1               163 / 0    124 / 0     29066 / 0        1172 / 0     12681 / 0    592 / 0
    empty-state updates                      0          0          1136               0           545         14
    signal-only / real-only states        0 / 355    0 / 449    1344 / 1736       0 / 548        0 / 0      0 / 0
    update_X uniform fallbacks               0          0            18               0             2          1
    categorical guard stops                  0          0             0               0             0          0

So the window that selects a kernel (T >= 129 on the register-resident ladder, the longest of the five on the LDS-resident
kernel) saw the identity order on 97 % of its sweeps and never a 3-cycle: a kernel that gathered A[order[i]][order[j]] through
the inverse permutation, or sorted the smoothed probabilities with the previous sweep's order, passed.  All the permuted sweeps
of the LDS-resident list are in its 2..257-step side windows, which the K <= 4 forms serve but which select nothing.  No
v <= 0 rejection, no gamma shape below one and no third attempt at site SIG2 had ever run on a GPU.

This module, same bar as everywhere (states bit-exact, floats within 1e-9 relative to 1 + |x|, through the C ABI):

  * test_mixed_labels_in_every_instantiation: one weakly separated window from a random start (branch_cases.py, "mixed") per
    instantiation of the coverage contract, at a length that selects it, the call's report asserted.  On the oracle the 185
    cases give: 1366 sweeps, 1306 with a non-identity order, 680 with an order that is not its own inverse; of 996 kept
    sweeps 953 and 521 (569 distinct orders).
  * test_directed_draw_branches: the table of branch_cases.py -- a third gamma attempt at SIG2 and at A, a v <= 0 rejection
    with a shape below one (alpha = 0.25), an empty state at T >= 1000 with the update_X uniform fallback, a signal-only and
    a real-only state -- in each place the draw code lives: the register-resident kernel's flavours p1, p2, h (K <= 4; there
    is no register-resident row at K >= 5, plan.hpp sends those to the LDS-resident kernel), the LDS-resident kernel in its
    LDS form (K = 5, 6) and in its streaming form (K = 5, 8, at the production length).  Of the families, only the LDS-resident
    one met the uniform fallback before (test_gpu_k8_edges.py, once); the empty-long rows add it to the other two.
    On the oracle the 25 rows give: 159 sweeps (156 permuted); third-or-later attempts 5 at SIG2 and 5 at A; 5 v <= 0
    rejections; 134 draws with a shape below one and 2075 with shape one; 145 empty-state updates; 10 signal-only and 15
    real-only states; 7 uniform fallbacks.

tests/test_branch_coverage.py (no GPU) holds both lists to the oracle's counters and the first to the instantiation set.
Not reachable, not tested: HMCG_ST_BAD_INVGAMMA (include/hmcg.h) and the categorical guard stop (cp <= u with every
probability added needs a law that sums below u < 1; the laws are normalised to within an ulp)."""
import numpy as np
import pytest

from hmc_jl_amd import _lib

import branch_cases as bc
from kernel_tables import FLAVOUR_WAVES
from oracle_parity import FLOAT_KEYS, TOL, assert_ran_on_big, assert_window_matches_oracle, close

pytestmark = pytest.mark.gpu

MIXED = bc.mixed_cases()
DIRECTED = bc.directed_cases()


def assert_intended_kernel_ran(c, g):
    if c.kind == "reg":
        K, L, path, fl = c.expect
        assert g["steps_per_thread"] == L and g["threads_per_window"] == 256, (g["steps_per_thread"], L)
        assert (g["helper_waves"], g["occupancy"]) == FLAVOUR_WAVES[fl] and g["buckets"] == 1
        assert not g["streaming"]
    elif c.kind == "sigsmooth":
        K, L = c.expect
        assert g["steps_per_thread"] == L and g["threads_per_window"] == 256 and g["helper_waves"] == 0
        assert g["occupancy"] == 1 and g["buckets"] == 1 and not g["streaming"]
    elif c.kind == "tpw":
        K, L, nt = c.expect
        assert g["threads_per_window"] == nt and g["steps_per_thread"] == L and g["buckets"] == 1
    else:
        sig, smooth, stream, K = c.expect
        assert_ran_on_big(g, stream, c.T, sig, smooth)


def run_and_compare(oracle, monkeypatch, c):
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    Y, yreal, x0 = bc.inputs(c)
    o = oracle.estimate_signals(Y, c.K, c.burnin, c.nrun, **bc.oracle_kwargs(c, yreal, x0))
    g = _lib.estimate_batch_host(Y[None, :], [c.T], c.K, c.burnin, c.nrun, bc.HORIZONS, yreal[None, :], **bc.gpu_kwargs(c, x0))
    assert_intended_kernel_ran(c, g)
    fields = FLOAT_KEYS + (("pi_smooth_mean", "pi_filter_mean") if c.smooth else ())
    if c.sig:
        fields += ("sigvals", "sample_summary")                               # (sigvals: the whole slab, as wide as the save range)
    elif c.smooth:
        fields += ("pi_smooth_draws",)                                        # samples.pib itself: (nd, T, K)
    assert_window_matches_oracle(g, 0, c.T, o, fields=fields)
    if not c.sig and not c.smooth:                                            # calccorr's matrix of the rounded draws (test_gpu_corr.py)
        cols = np.concatenate([o["mu"].T, o["sig2"].T, o["pi_end"].T, np.transpose(o["A"], (2, 1, 0)).reshape(c.K * c.K, -1), o["fcast"].T[:1]])
        with np.errstate(invalid="ignore", divide="ignore"):
            want = np.corrcoef(np.round(cols, 5))
        have = g["corr"][0]
        assert np.array_equal(np.isfinite(have), np.isfinite(want)), "corr: the constant columns differ"
        ok = np.isfinite(want)
        assert close(have[ok], want[ok]) < TOL, ("corr", close(have[ok], want[ok]))
    return g, o


@pytest.mark.parametrize("case", MIXED, ids=[c.id for c in MIXED])
def test_mixed_labels_in_every_instantiation(hmclib, oracle, monkeypatch, case):
    g, o = run_and_compare(oracle, monkeypatch, case)
    assert not bc.mixed_conditions(case, o["branches"], o["status"])          # (test_branch_coverage.py says so without a GPU)
    mu = o["mu"]
    assert (np.diff(g["mu"][0].T, axis=1) > 0).all() and (np.diff(mu, axis=1) > 0).all()      # labels sorted on every draw


@pytest.mark.parametrize("case", DIRECTED, ids=[c.id for c in DIRECTED])
def test_directed_draw_branches(hmclib, oracle, monkeypatch, case):
    g, o = run_and_compare(oracle, monkeypatch, case)
    assert not bc.directed_conditions(case, o["branches"], o["status"])
