"""The helper flavour's parameter phase: the transition counts are published first, wave 0 draws everything that depends on
them alone while the pivoted state sums finish beside it (its own four steps' sums on helper wave 4), and the sig2 / mu
lanes complete after one more barrier.  Every value keeps its expression tree and summation order, so the helper flavour
`h` must equal the plain flavour `p1` -- which takes the statistics in one piece -- BIT FOR BIT, and both the oracle.

Lengths: T = 2; T = 37 (every real step on wave 0: the helper wave computes all the sums); 63, 64, 65 (wave 0 one short of
full, exactly full, one step on wave 1); 256 L - 1 for L = 2, 4, 8.  The six-barrier loop is compiled for four steps per
thread (T = 1023 here, and the short windows of the two tests that run one unbucketed launch); the other rows of CASES
select other steps-per-thread classes, whose kernels this change leaves as they were: regression pins of the helper
flavour's five-barrier loop, not tests of the new one."""
import numpy as np
import pytest

from hmc_jl_amd import _lib, synth
from kernel_tables import steps_per_thread
from oracle_parity import assert_same, assert_window_matches_oracle, forced_flavour_call

pytestmark = pytest.mark.gpu
KEYS = ("mu", "sig2", "A", "pi_end", "fcast", "summary", "x_final", "status")
LENGTHS = [2, 37, 63, 64, 65, 511, 1023, 2047]
CASES = [(K, T) for K in (2, 3, 4) for T in LENGTHS]
BURNIN, NRUN, HORIZONS = 2, 10, (1, 12)


_panels, _runs = {}, {}


def panel(K, T):
    if (K, T) not in _panels:
        Y, Tw, fut = synth.generate_panel(2, T, K)
        _panels[K, T] = (Y, Tw, fut[:, [0, 11]], np.array([5, 11]))
    return _panels[K, T]


def run(monkeypatch, flavour, K, T, **kw):
    """One free chain of the (K, T) panel under the forced flavour; the full-length runs are shared between the tests."""
    key = (flavour, K, T) if not kw else None
    if key in _runs:
        return _runs[key]
    Y, Tw, yreal, ids = panel(K, T)
    g = forced_flavour_call(monkeypatch, flavour, Y, Tw, K, BURNIN, NRUN, HORIZONS, yreal, window_ids=ids, **kw)
    assert g["steps_per_thread"] == steps_per_thread(K, T) and g["threads_per_window"] == 256
    assert not (g["status"] & _lib.ST_SKIPPED).any()
    if key:
        _runs[key] = g
    return g


def against_oracle(oracle, g, Y, lens, K, yreal, ids):
    for w, T in enumerate(lens):
        o = oracle.estimate_window(Y[w, :T], K, BURNIN, NRUN, HORIZONS, yreal[w], window_id=int(ids[w]))
        assert_window_matches_oracle(g, w, T, o, fields=("mu", "sig2", "A", "pi_end", "fcast", "summary"), status0=False)


@pytest.mark.parametrize("K,T", CASES, ids=["K%d-T%d" % c for c in CASES])
def test_helper_flavour_equals_plain_bit_for_bit(hmclib, monkeypatch, K, T):
    assert_same(run(monkeypatch, "h", K, T), run(monkeypatch, "p1", K, T), KEYS, equal_nan=False)


@pytest.mark.parametrize("K,T", CASES, ids=["K%d-T%d" % c for c in CASES])
def test_helper_flavour_against_oracle(hmclib, oracle, monkeypatch, K, T):
    Y, Tw, yreal, ids = panel(K, T)
    against_oracle(oracle, run(monkeypatch, "h", K, T), Y, [T, T], K, yreal, ids)


@pytest.mark.parametrize("T", [37, 511, 1023])
def test_launch_split_between_counts_and_sums(hmclib, monkeypatch, T):
    """3 + 4 sweeps resumed == 7 sweeps in one launch: the resumed launch's prologue takes counts AND sums on the window's
    own waves, and its first sweep must find both ready (no sums pass, no count pass of a previous sweep to rely on)."""
    monkeypatch.setenv("HMCG_FLAVOUR", "h")
    Y, Tw, yreal, ids = panel(3, T)
    args, kw = (Y, Tw, 3, 2, 5, HORIZONS, yreal), dict(window_ids=ids, want_state=True)
    one = _lib.estimate_batch_host(*args, **kw)
    a = _lib.estimate_batch_host(*args, sweep_count=3, **kw)
    b = _lib.estimate_batch_host(*args, resume_state=a, sweep_base=3, **kw)
    assert one["helper_waves"] == a["helper_waves"] == b["helper_waves"] == 4
    for k in ("mu", "sig2", "pi_end", "fcast"):
        assert np.array_equal(a[k][:, :, :1], one[k][:, :, :1]), k          # draw 0 = sweep 2, from the first launch
        assert np.array_equal(b[k][:, :, 1:], one[k][:, :, 1:]), k
    assert np.array_equal(a["A"][..., :1], one["A"][..., :1]) and np.array_equal(b["A"][..., 1:], one["A"][..., 1:])
    assert np.array_equal(b["summary"], one["summary"])
    assert np.array_equal(b["x_final"], one["x_final"])


@pytest.mark.parametrize("K,T", [(3, 2), (4, 2), (4, 3)])
def test_state_never_visited(hmclib, monkeypatch, K, T):
    """T < K: on every sweep at least one state has no step at all (its count is 0: the sig2 lane's `c > 0` guards, before
    and after Ba2, and a transition pair never seen draws Gamma(1) through the `shape == 1` branch), over 20 sweeps, ON the
    six-barrier kernel: a T = 1023 companion window and one unbucketed launch put the short window on four steps per thread."""
    Y, Tw, fut = synth.generate_panel(2, 1023, K, ragged=[1023, T])
    yreal, ids = fut[:, [0, 11]], np.array([7, 13])
    monkeypatch.setenv("HMCG_NO_BUCKETS", "1")
    out = {}
    for fl in ("h", "p1"):
        out[fl] = g = forced_flavour_call(monkeypatch, fl, Y, Tw, K, 4, 16, HORIZONS, yreal, window_ids=ids)
        assert g["steps_per_thread"] == 4 and g["buckets"] == 1
        assert not (g["status"] & _lib.ST_SKIPPED).any()
    assert_same(out["h"], out["p1"], KEYS, equal_nan=False)
    assert np.isfinite(out["h"]["mu"]).all() and np.isfinite(out["h"]["A"]).all()


@pytest.mark.parametrize("K", [2, 3, 4])
def test_short_windows_on_the_four_step_kernel(hmclib, oracle, monkeypatch, K):
    """The same edge cases ON the six-barrier kernel: one launch sized for the longest window (T = 1023: four steps per
    thread) runs windows whose real steps all lie on wave 0 -- T = 2, 37 (the helper wave computes every sum that is not
    zero), 255, 256 (wave 0 one short of full, exactly full) -- and T = 257 (one step on wave 1).  `h` against `p1` bit
    for bit, and against the oracle."""
    lens = [1023, 2, 37, 255, 256, 257]
    Y, Tw, fut = synth.generate_panel(len(lens), max(lens), K, ragged=lens)
    yreal, ids = fut[:, [0, 11]], np.arange(20, 20 + len(lens))
    monkeypatch.setenv("HMCG_NO_BUCKETS", "1")
    out = {}
    for fl in ("h", "p1"):
        out[fl] = g = forced_flavour_call(monkeypatch, fl, Y, Tw, K, BURNIN, NRUN, HORIZONS, yreal, window_ids=ids)
        assert g["steps_per_thread"] == 4 and g["buckets"] == 1
        assert not (g["status"] & _lib.ST_SKIPPED).any()
    assert_same(out["h"], out["p1"], KEYS, equal_nan=False)
    against_oracle(oracle, out["h"], Y, lens, K, yreal, ids)
