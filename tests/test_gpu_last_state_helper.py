"""X[T-1] drawn by a helper wave between Bd and Be (gibbs_device.hpp, HELPER_DRAW): in the six-barrier helper rows of K = 2 and
of K = 3 on the base path, four steps per thread, the maps of step T-1 and of the padded slots are the identity, helper
DRAW_WAVE draws the state from th.mu, th.pi_end and the step's uniform in LDS and stores sh.x_end ahead of Be, and behind Be the
own waves apply their composed suffix to it: slot T-1 takes it through the identity, the slots behind it take the padding
value by a select.  tests/test_gpu_last_state.py holds the owner's form of every class; this module holds the new form to the
oracle where it can go wrong: the slot, lane and wave of step T-1 and the padding behind it.

Every comparison goes through the C ABI against the oracle: states array_equal, floats within oracle_parity.TOL = 1e-9.
The calls are unbucketed (HMCG_NO_BUCKETS) launches of up to three ragged windows, 2 burn-in and 12 kept sweeps, K = 2 and 3,
with HMCG_FLAVOUR=h forced and, separately, with the table's own choice.  LENGTHS is the case table; the test at the end of the
file, which needs no GPU, holds it to its contract (slot, lane and padding coverage computed from T, K and L)."""
import numpy as np
import pytest

import kernel_tables as kt
from hmc_jl_amd import _lib, synth
from oracle_parity import assert_same, assert_window_matches_oracle, check_smoothing_against_oracle, forced_flavour_call

gpu = pytest.mark.gpu
L, NT = 4, kt.NT                                   # the four-steps class: T = 769..1024 on 256 threads
BURNIN, NRUN, HORIZONS = 2, 12, (1, 12)
FLOATS = ("mu", "sig2", "A", "pi_end", "fcast", "summary")
KEYS = FLOATS + ("x_final", "status")
KS = (2, 3)
FLAVOURS = ("h", None)                             # forced helper flavour | the table's own choice
# one launch per row, at most three windows each
LENGTHS = (
    (769, 770, 1024),           # step T-1 in slot 0 of lane 0 of the last wave | slot 1 | slot 3 of the last lane: no padding at all
    (771, 772, 1000),           # slot 2 | slot 3, 252 padded slots behind it | the headline: 24 padded slots, six threads of padding
    (1021, 1022, 1023),         # 3, 2, 1 padded slots inside the owner's own thread
)
SMOOTH_LENGTHS = (1000, 1023)
RESUME_ROW, RESUME_CUT = 1, 5                      # 14 sweeps == 5 + 9 resumed: the cut lies among the kept sweeps
CASES = [(K, row) for K in KS for row in range(len(LENGTHS))]
IDS = ["K%d-T%s" % (K, "_".join(map(str, LENGTHS[row]))) for K, row in CASES]


def owner(T):
    """(wave, lane, slot) of step T-1 and the padded slots behind it: in the owner's thread, in all."""
    tid, slot = divmod(T - 1, L)
    return tid // 64, tid % 64, slot, L - 1 - slot, NT * L - T


_panels, _oracle = {}, {}


def panel(K, row):
    if (K, row) not in _panels:
        lens = LENGTHS[row]
        Y, Tw, fut = synth.generate_panel(len(lens), max(lens), K, ragged=lens)
        _panels[K, row] = (Y, Tw, np.ascontiguousarray(fut[:, [0, 11]]), np.arange(70, 70 + len(lens)))
    return _panels[K, row]


def reference(oracle, K, row):
    """The oracle's runs of the row's windows, once per (K, row)."""
    if (K, row) not in _oracle:
        Y, Tw, yreal, ids = panel(K, row)
        _oracle[K, row] = [oracle.estimate_window(Y[w, :T], K, BURNIN, NRUN, HORIZONS, yreal[w], window_id=int(ids[w])) for w, T in enumerate(Tw)]
    return _oracle[K, row]


@gpu
@pytest.mark.parametrize("flavour", FLAVOURS, ids=["h", "table"])
@pytest.mark.parametrize("K,row", CASES, ids=IDS)
def test_last_step_against_oracle(hmclib, oracle, monkeypatch, K, row, flavour):
    monkeypatch.setenv("HMCG_NO_BUCKETS", "1")
    Y, Tw, yreal, ids = panel(K, row)
    g = forced_flavour_call(monkeypatch, flavour, Y, Tw, K, BURNIN, NRUN, HORIZONS, yreal, window_ids=ids)
    assert g["steps_per_thread"] == L and g["threads_per_window"] == NT and g["buckets"] == 1
    ref = reference(oracle, K, row)
    for w, T in enumerate(Tw):
        assert_window_matches_oracle(g, w, int(T), ref[w], fields=FLOATS)


@gpu
@pytest.mark.parametrize("K", KS)
def test_resumed_launches_equal_one(hmclib, monkeypatch, K):
    """The same call as two launches (the second resumed from the first one's checkpoint) equals the single launch bit for
    bit: the first sweep of either launch takes X[T-1] from the prologue, every later one from the helper's draw."""
    monkeypatch.setenv("HMCG_NO_BUCKETS", "1")
    monkeypatch.setenv("HMCG_FLAVOUR", "h")
    Y, Tw, yreal, ids = panel(K, RESUME_ROW)
    args, kw = (Y, Tw, K, BURNIN, NRUN, HORIZONS, yreal), dict(want_state=True, window_ids=ids)
    one = _lib.estimate_batch_host(*args, **kw)
    a = _lib.estimate_batch_host(*args, sweep_count=RESUME_CUT, **kw)
    b = _lib.estimate_batch_host(*args, resume_state=a, sweep_base=RESUME_CUT, **kw)
    for g in (one, a, b):
        assert g["steps_per_thread"] == L and g["helper_waves"] == 4
    kept = RESUME_CUT - BURNIN                                      # draws the first launch kept
    for k in ("mu", "sig2", "pi_end", "fcast"):
        assert np.array_equal(a[k][:, :, :kept], one[k][:, :, :kept]), k
        assert np.array_equal(b[k][:, :, kept:], one[k][:, :, kept:]), k
    assert np.array_equal(a["A"][..., :kept], one["A"][..., :kept]) and np.array_equal(b["A"][..., kept:], one["A"][..., kept:])
    assert_same(b, one, ("summary", "x_final", "status"), equal_nan=False)


@gpu
@pytest.mark.parametrize("K,form", [(2, "new"), (3, "parent's")], ids=["K2-new-form", "K3-parents-form"])
def test_smoothed_means(hmclib, oracle, monkeypatch, K, form):
    """pi_smooth_mean requested, helper flavour: the K = 2 row takes the new form, the K = 3 row (register-capped) the parent's."""
    monkeypatch.setenv("HMCG_NO_BUCKETS", "1")
    monkeypatch.setenv("HMCG_FLAVOUR", "h")
    Y, Tw, fut = synth.generate_panel(len(SMOOTH_LENGTHS), max(SMOOTH_LENGTHS), K, ragged=SMOOTH_LENGTHS)
    g = check_smoothing_against_oracle(oracle, Y, Tw, K, BURNIN, NRUN, np.ascontiguousarray(fut[:, 11:12]))
    assert g["steps_per_thread"] == L and g["helper_waves"] == 4


# ---- the contract of the table above: no GPU ----
def test_case_table_covers_what_it_claims():
    import test_variant_coverage as cov
    lens = [T for row in LENGTHS for T in row]
    assert all(len(row) <= 3 for row in LENGTHS) and len(SMOOTH_LENGTHS) <= 3 and (BURNIN, NRUN) == (2, 12)
    for K in KS:                                                     # every length, and every row's longest, selects the four-steps class
        assert all(kt.steps_per_thread(K, T) == L for T in lens + list(SMOOTH_LENGTHS)), K
        assert (K, L, "base") in kt.VARIANT_ROWS                     # ... which exists in the helper flavour
        assert all(NT * (L - 1) < T <= NT * L for T in lens)
    assert {owner(T)[2] for T in lens} == {0, 1, 2, 3}               # step T-1 in every slot
    assert owner(1024) == (3, 63, 3, 0, 0) and 1024 in lens          # the last lane of the last wave: no padding at all
    assert owner(769)[:3] == (3, 0, 0) and 769 in lens               # lane 0 of the last wave
    assert owner(1000)[3:] == (0, 24) and 1000 in lens               # the headline: 24 padded slots, none in the owner's thread
    assert [owner(T)[3:] for T in (1021, 1022, 1023)] == [(3, 3), (2, 2), (1, 1)] and {1021, 1022, 1023} <= set(lens)
    assert any(owner(T)[4] >= L + owner(T)[3] for T in lens)         # whole threads of padding behind the owner
    assert 1000 in LENGTHS[RESUME_ROW] and BURNIN < RESUME_CUT < BURNIN + NRUN
    # smoothing: both K have the helper row at four steps; only K = 2 holds its registers with the owner's form and so takes the new one
    assert (2, L, "smooth") in kt.VARIANT_ROWS and (3, L, "smooth") in kt.VARIANT_ROWS
    assert [c[0] for c in cov.cases_of(test_smoothed_means)] == [2, 3]
    assert any(owner(T)[3] for T in SMOOTH_LENGTHS) and 1000 in SMOOTH_LENGTHS
    assert list(cov.cases_of(test_resumed_launches_equal_one)) == list(KS)
