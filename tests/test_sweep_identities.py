"""The oracle's sampling loop against the reference's formulas, without a GPU: what one sweep of oracle/hmc_oracle.c reports --
its filtered probabilities, the smoothed rows per step, the row reported as pi_end (at end_pos when signals run past the end
date, sigLen > 0), the forecasts and the forecastsignal blend -- recomputed in numpy.longdouble from the run's own outputs by
tests/sweep_identities.py, over the case table the GPU suite runs on every smoothing-capable kernel form
(tests/test_gpu_sweep_identities.py).  This is the independent pin of the oracle's sigLen > 0 reporting and of its in-loop smoother;
its two stand-alone kernels are pinned by tests/test_oracle_kernels.py.

Bound: 1e-11 on each of the four residuals, the bound of tests/test_config_range_cases.py's long-double check.  Largest values over
the table (K = 2..8, T = 64..7935, sigLen 0, 1, 12, 100, 256 and all-signal, burn-in 0..3; 37 cases, 109 windows):
    filter step 1.0e-15   smoother 2.5e-14   reported row 4.1e-15 (0 without end_pos)   forecasts and blend 5.7e-16
The smallest filtered probability is 9.0e-176 (> 0: no ratio is 0/0, no step of any window is left out).

Then the checker itself: each of six deliberately wrong inputs must raise a residual to >= 1e-6, 1000 x the GPU suite's
tolerance, on a case where that feature is live."""
import numpy as np
import pytest

import sweep_identities as si
from hmc_jl_amd import _lib

BOUND = 1e-11
CAUGHT = 1e-6


def test_table_constants():
    assert si.MAXTAIL == _lib.HMCG_MAXTAIL
    assert len(set(si.CASE_IDS)) == len(si.CASES)
    assert {c["burnin"] for c in si.CASES} == {0, 1, 2, 3}
    for c in si.CASES:
        assert 2 <= len(c["lens"]) <= 3 and len(set(c["window_ids"])) == len(c["lens"]), c["id"]
        if c["path"] == "tail+smooth":
            assert set(c["ssig"]) <= {0.4, 1.3}, c["id"]                 # never 1.0: there a = 1 - a
    tails = {n for c in si.CASES if c["tail"] for n in c["tail"]}
    assert tails >= {1, 12, si.MAXTAIL}


@pytest.mark.parametrize("c", si.CASES, ids=si.CASE_IDS)
def test_oracle_meets_the_identities(oracle, c):
    args, kw, runs = si.oracle_runs(oracle, c)
    for w, o in enumerate(runs):
        pos, wkw = si.oracle_inputs(args, kw, w, o)
        r = si.residuals(*pos, **wkw)
        what = "%s window %d (T = %d): %s" % (c["id"], w, c["lens"][w], si.describe(r))
        print(what)
        assert o["status"] == 0, what
        assert r["min_pif"] > 0 and r["left_out"] == 0, what
        for k in si.IDENTITIES:
            assert r[k] <= BOUND, what
        # pib[T-1] = pif[T-1] (:448), and without end_pos that row is what pi_end reports
        assert np.array_equal(o["pi_smooth"][0][-1], o["pi_filter_mean"][-1])
        if "end_pos" not in kw:
            assert np.array_equal(o["pi_end"][0], o["pi_filter_mean"][-1])


# ---- the checker can fail ----
def _mutated(oracle, ids, mutate):
    """The largest residual per identity over the windows of the cases `ids`, with mutate(pos, kw) -> (pos, kw) applied to
    residuals()'s arguments."""
    worst = dict.fromkeys(si.IDENTITIES, 0.0)
    for id in ids:
        args, kw, runs = si.oracle_runs(oracle, si.case_by_id(id))
        for w, o in enumerate(runs):
            pos, wkw = si.oracle_inputs(args, kw, w, o)
            pos, wkw = mutate(list(pos), dict(wkw))
            r = si.residuals(*pos, **wkw)
            for k in si.IDENTITIES:
                worst[k] = max(worst[k], r[k])
    return worst


SIG_LIVE = ("reg-sigsm-K3-L2", "reg-sigsm-K3-allsignal", "lds-sigsm-K6")
TAIL_LIVE = ("reg-tailsm-K2-L1", "reg-tailsm-K3-L4", "lds-tailsm-K5", "lds-tailsm-K8")
ANY = ("reg-sm-K2-L1-p1", "lds-sm-K5", "reg-tailsm-K3-L4")
A_, PIF, PIB = 2, 3, 4                     # positions among residuals()'s arguments


def _without_kappa(pos, kw):
    kw["kappa"] = 0.0
    return pos, kw


def _a_transposed(pos, kw):
    pos[A_] = pos[A_].T
    return pos, kw


def _same_step_predecessor(pos, kw):
    kw["lag"] = 0
    return pos, kw


def _end_pos_off_by_one(pos, kw):
    kw["end_pos"] -= 1
    return pos, kw


def _wrong_blend_weight(pos, kw):
    kw["sigma_signal"] = 1.0 / kw["sigma_signal"]          # tau and 1 / tau change places: a becomes 1 / (1 + tau)
    return pos, kw


def _one_pif_entry_moved(pos, kw):
    # the entry the smoother leans on most: the backward step divides by pif[t,s], so moving it by d moves the row before by
    # about pib[t,s] d / (pif[t,s] + d) -- largest where smoothing raises a state the filter had all but excluded
    pif = np.array(pos[PIF])
    t, s = np.unravel_index(np.argmax(pos[PIB][1:] / (pif[1:] + 1e-7)), pif[1:].shape)
    pif[t + 1, s] += 1e-7
    pos[PIF] = pif
    return pos, kw


MUTATIONS = [
    ("(1 + kappa) left out", SIG_LIVE, _without_kappa, "filter"),
    ("A transposed", ANY, _a_transposed, "filter"),
    ("pif[t] where pif[t-1] belongs", ANY, _same_step_predecessor, "filter"),
    ("end_pos off by one", TAIL_LIVE, _end_pos_off_by_one, "row"),
    ("a = 1 / (1 + tau)", TAIL_LIVE, _wrong_blend_weight, "forecast"),
    ("one pif entry moved by 1e-7", ANY + TAIL_LIVE, _one_pif_entry_moved, "smoother"),
]


@pytest.mark.parametrize("name,ids,mutate,shows_in", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_checker_catches(oracle, name, ids, mutate, shows_in):
    clean = _mutated(oracle, ids, lambda pos, kw: (pos, kw))
    assert max(clean.values()) <= BOUND, clean
    worst = _mutated(oracle, ids, mutate)
    print(name, worst)
    assert worst[shows_in] >= CAUGHT, (name, worst)
