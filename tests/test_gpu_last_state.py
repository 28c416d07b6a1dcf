"""X[T-1], the state of the last step, in the K <= 4 sweep (gibbs_device.hpp): in the rows that hold their registers the
thread that owns step T-1 draws it ahead of barrier Bd from the filtered probabilities and the uniform it holds in registers,
keeps it for its own map of step T-1 and writes sh.x_end for wave 0's next parameter phase itself; the other rows publish the
uniform and every thread draws the state behind Bd.  Behind Be the later waves' maps are fetched with one wait.

What can go wrong depends on WHERE step T-1 lies: which wave, which lane (the first and the last of a wave), which slot of the
thread, and whether padding follows.  A class's own length range does not put it everywhere, so the calls are unbucketed
(HMCG_NO_BUCKETS): one ragged launch per steps-per-thread class L runs the windows

    L = 1    64, 65, 128, 129, 192, 193, 255, 256              lane 63 or lane 0 of each wave, and no padding at all
    L = 2    257, 258, 383, 384, 385, 511, 512
    L = 3    513, 514, 515, 766, 767, 768
    L = 4    769, 770, 771, 772, 1021, 1022, 1023, 1024         every slot of the owner
    L = 8    1025, 2041 .. 2048

(the longest selects the class; the classes of fewer than eight lengths repeat their first ones up to eight windows, L = 8
has nine), 4 burn-in and 16 kept sweeps, K = 2, 3, 4, flavours h, p1, p2: equal bit for bit, and each against the oracle
with the states exact and every float within 1e-9.  The eight-wave row runs T = 1000 through threads_per_window = 512.

X[T-1] crosses a checkpoint in the state path and the sweep bounds differ from launch to launch: 12 sweeps in one launch
equal 1 + 11 and 5 + 7 resumed, bit for bit.  The signal path (K = 3, T = 771, three noise samples) is held to the oracle as
tests/test_gpu_parity.py holds its signal cases."""
import numpy as np
import pytest

from hmc_jl_amd import _lib, synth
from kernel_tables import register_classes
from oracle_parity import assert_same, assert_window_matches_oracle, check_signals_against_oracle, forced_flavour_call

pytestmark = pytest.mark.gpu
W, BURNIN, NRUN, HORIZONS = 8, 4, 16, (1, 12)
FLOATS = ("mu", "sig2", "A", "pi_end", "fcast", "summary")
KEYS = FLOATS + ("x_final", "status")
FLAVOURS = ("h", "p1", "p2")
LENGTHS = {
    1: [64, 65, 128, 129, 192, 193, 255, 256],
    2: [257, 258, 383, 384, 385, 511, 512],
    3: [513, 514, 515, 766, 767, 768],
    4: [769, 770, 771, 772, 1021, 1022, 1023, 1024],
    8: [1025] + list(range(2041, 2049)),
}
CASES = [(K, L) for K in (2, 3, 4) for L in sorted(LENGTHS) if L in register_classes(K, False, False)]
IDS = ["K%d-L%d" % c for c in CASES]


def windows(L):
    lens = LENGTHS[L]
    return lens + lens[:max(0, W - len(lens))]


_panels, _runs, _oracle = {}, {}, {}


def panel(K, L):
    if (K, L) not in _panels:
        lens = windows(L)
        Y, Tw, fut = synth.generate_panel(len(lens), max(lens), K, ragged=lens)
        _panels[K, L] = (Y, Tw, np.ascontiguousarray(fut[:, [0, 11]]), np.arange(40, 40 + len(lens)))
    return _panels[K, L]


def run(monkeypatch, flavour, K, L):
    if (flavour, K, L) not in _runs:
        monkeypatch.setenv("HMCG_NO_BUCKETS", "1")
        Y, Tw, yreal, ids = panel(K, L)
        g = forced_flavour_call(monkeypatch, flavour, Y, Tw, K, BURNIN, NRUN, HORIZONS, yreal, window_ids=ids)
        assert g["steps_per_thread"] == L and g["threads_per_window"] == 256 and g["buckets"] == 1
        assert not (g["status"] & _lib.ST_SKIPPED).any()
        _runs[flavour, K, L] = g
    return _runs[flavour, K, L]


def reference(oracle, K, L):
    """The oracle's runs of the panel's windows, once per (K, L)."""
    if (K, L) not in _oracle:
        Y, Tw, yreal, ids = panel(K, L)
        _oracle[K, L] = [oracle.estimate_window(Y[w, :T], K, BURNIN, NRUN, HORIZONS, yreal[w], window_id=int(ids[w])) for w, T in enumerate(Tw)]
    return _oracle[K, L]


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("K,L", CASES, ids=IDS)
def test_last_step_on_every_owner_against_oracle(hmclib, oracle, monkeypatch, K, L, flavour):
    ref = reference(oracle, K, L)
    g = run(monkeypatch, flavour, K, L)
    for w, T in enumerate(panel(K, L)[1]):
        assert_window_matches_oracle(g, w, int(T), ref[w], fields=FLOATS)


@pytest.mark.parametrize("K,L", CASES, ids=IDS)
def test_last_step_flavours_equal_bit_for_bit(hmclib, monkeypatch, K, L):
    h = run(monkeypatch, "h", K, L)
    assert_same(h, run(monkeypatch, "p1", K, L), KEYS, equal_nan=False)
    assert_same(h, run(monkeypatch, "p2", K, L), KEYS, equal_nan=False)


def test_last_step_on_the_eight_wave_row(hmclib, oracle, monkeypatch):
    """T = 1000 on 512 threads: two steps per thread, the owner of step 999 is lane 51 of wave 7."""
    K, T = 3, 1000
    Y, Tw, fut = synth.generate_panel(W, T, K)
    yreal = np.ascontiguousarray(fut[:, [0, 11]])
    monkeypatch.setenv("HMCG_NO_BUCKETS", "1")
    g = forced_flavour_call(monkeypatch, None, Y, Tw, K, BURNIN, NRUN, HORIZONS, yreal, threads_per_window=512)
    assert g["steps_per_thread"] == 2 and g["threads_per_window"] == 512 and g["buckets"] == 1
    for w in range(W):
        o = oracle.estimate_window(Y[w], K, BURNIN, NRUN, HORIZONS, yreal[w], window_id=w)
        assert_window_matches_oracle(g, w, T, o, fields=FLOATS)


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("T,L", [(256, 1), (771, 4), (1024, 4)])
def test_last_state_crosses_a_checkpoint(hmclib, monkeypatch, K, T, L):
    """12 sweeps (4 burn-in + 8 kept) in one launch == 1 + 11 == 5 + 7 resumed from the checkpoint, in every flavour: the resumed
    launch's X[T-1] comes from the state path, and its sweep bounds are not the first launch's."""
    burnin, nrun = 4, 8
    Y, Tw, fut = synth.generate_panel(W, T, K)
    args, kw = (Y, Tw, K, burnin, nrun, HORIZONS, np.ascontiguousarray(fut[:, [0, 11]])), dict(want_state=True)
    for fl in FLAVOURS:
        monkeypatch.setenv("HMCG_FLAVOUR", fl)
        one = _lib.estimate_batch_host(*args, **kw)
        assert one["steps_per_thread"] == L and one["helper_waves"] == (4 if fl == "h" else 0)
        for cut in (1, 5):
            a = _lib.estimate_batch_host(*args, sweep_count=cut, **kw)
            b = _lib.estimate_batch_host(*args, resume_state=a, sweep_base=cut, **kw)
            assert a["steps_per_thread"] == b["steps_per_thread"] == L
            kept = max(0, cut - burnin)                        # draws the first launch kept
            for k in ("mu", "sig2", "pi_end", "fcast"):
                assert np.array_equal(a[k][:, :, :kept], one[k][:, :, :kept]), (fl, cut, k)
                assert np.array_equal(b[k][:, :, kept:], one[k][:, :, kept:]), (fl, cut, k)
            assert np.array_equal(a["A"][..., :kept], one["A"][..., :kept]) and np.array_equal(b["A"][..., kept:], one["A"][..., kept:]), (fl, cut)
            assert np.array_equal(b["summary"], one["summary"]), (fl, cut)
            assert np.array_equal(b["x_final"], one["x_final"]), (fl, cut)
            assert np.array_equal(b["status"], one["status"]), (fl, cut)


def test_last_state_on_the_signal_path(hmclib, oracle):
    """K = 3, T = 771 (four steps per thread, step T-1 in the owner's third slot), three noise samples: a tail of signals, one
    signal step, half the window."""
    K, T = 3, 771
    Y, Tw, fut = synth.generate_panel(3, T, K)
    sig = np.array([[T - 40, T], [T - 1, T], [T // 2, T]]); save = np.array([[T - 3, T], [T - 1, T], [T - 2, T]])
    g = check_signals_against_oracle(oracle, Y, Tw, K, 3, 8, 3, sig, save, 0.6, 2.0, 2.0, np.array([0.5, 1.0, 0.2]), fut[:, 11:12])
    assert g["steps_per_thread"] == 4
