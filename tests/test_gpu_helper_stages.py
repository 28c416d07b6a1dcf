"""The helper flavour's staged helper jobs (the six `<K,4,256,false,SMOOTH,4,2>` kernels): the next sweep's RNG preparation
is cut in time at barrier Bc -- Philox block, u53 and the log before it; Box-Muller, the rho normalisation and the stores
behind it, with r[2], r[3], uraw and lg carried in registers across the barrier.  Beside it, on helper 4, runs the fourth
uniform trip, generated a sweep ahead into the other uniform buffer.  Every value keeps its Philox counter and expression
tree, so `h` must equal the plain flavour `p1` BIT FOR BIT, and both the oracle (states exact, floats to 1e-9).

A trip is 128 Philox blocks of two steps; the ahead trip covers blocks 384..511 (two blocks per lane: t = 768..895 and
896..1023).  Lengths: 769 (one block of the first 64, none of the second), 895, 896, 897 (first block of the second 64),
1023, 1024 (last block full).  Every launch here runs four steps per thread; two windows each."""
import numpy as np
import pytest

from hmc_jl_amd import _lib, synth
from oracle_parity import assert_same, assert_window_matches_oracle, forced_flavour_call

pytestmark = pytest.mark.gpu
KEYS = ("mu", "sig2", "A", "pi_end", "fcast", "summary", "x_final", "status")
LENGTHS = [769, 895, 896, 897, 1023, 1024]
CASES = [(K, T) for K in (2, 3, 4) for T in LENGTHS]
BURNIN, NRUN, HORIZONS = 2, 10, (1, 12)


_panels, _runs = {}, {}


def panel(K, T):
    if (K, T) not in _panels:
        Y, Tw, fut = synth.generate_panel(2, T, K)
        _panels[K, T] = (Y, Tw, fut[:, [0, 11]], np.array([5, 11]))
    return _panels[K, T]


def call(monkeypatch, flavour, K, T, burnin=BURNIN, nrun=NRUN, **kw):
    """One call on the (K, T) panel under the forced flavour, on the four-steps-per-thread kernel."""
    Y, Tw, yreal, ids = panel(K, T)
    g = forced_flavour_call(monkeypatch, flavour, Y, Tw, K, burnin, nrun, HORIZONS, yreal, window_ids=ids, **kw)
    assert g["steps_per_thread"] == 4 and g["threads_per_window"] == 256
    assert not (g["status"] & _lib.ST_SKIPPED).any()
    return g


def run(monkeypatch, flavour, K, T):
    """The full-length free chain, shared between the tests."""
    if (flavour, K, T) not in _runs:
        _runs[flavour, K, T] = call(monkeypatch, flavour, K, T)
    return _runs[flavour, K, T]


def against_oracle(oracle, g, Y, lens, K, burnin, nrun, yreal, ids, fields=("mu", "sig2", "A", "pi_end", "fcast", "summary"), **want):
    for w, T in enumerate(lens):
        o = oracle.estimate_window(Y[w, :T], K, burnin, nrun, HORIZONS, yreal[w], window_id=int(ids[w]), **want)
        assert_window_matches_oracle(g, w, T, o, fields=fields, status0=False)


@pytest.mark.parametrize("K,T", CASES, ids=["K%d-T%d" % c for c in CASES])
def test_trip_edges_equal_plain_bit_for_bit(hmclib, monkeypatch, K, T):
    assert_same(run(monkeypatch, "h", K, T), run(monkeypatch, "p1", K, T), KEYS, equal_nan=False)


@pytest.mark.parametrize("K,T", CASES, ids=["K%d-T%d" % c for c in CASES])
def test_trip_edges_against_oracle(hmclib, oracle, monkeypatch, K, T):
    Y, Tw, yreal, ids = panel(K, T)
    against_oracle(oracle, run(monkeypatch, "h", K, T), Y, [T, T], K, BURNIN, NRUN, yreal, ids)


@pytest.mark.parametrize("burnin,nrun", [(0, 1), (1, 1), (1, 2)], ids=["1-sweep", "2-sweeps", "3-sweeps"])
def test_sweep_counts_at_which_a_stage_could_dangle(hmclib, oracle, monkeypatch, burnin, nrun):
    """1, 2 and 3 sweeps in all: a launch's last sweep starts no preparation (there is no next sweep) and leaves none half
    done; a one-sweep launch runs no stage at all, a two-sweep launch exactly one of each."""
    K, T = 3, 897
    h = call(monkeypatch, "h", K, T, burnin, nrun)
    assert_same(h, call(monkeypatch, "p1", K, T, burnin, nrun), KEYS, equal_nan=False)
    Y, Tw, yreal, ids = panel(K, T)
    against_oracle(oracle, h, Y, [T, T], K, burnin, nrun, yreal, ids)


@pytest.mark.parametrize("parts", [(1, 1, 1), (3, 4)], ids=["1+1+1", "3+4"])
def test_resumed_chains_at_both_buffer_parities(hmclib, monkeypatch, parts):
    """Launches of 1 + 1 + 1 sweeps against 3, and 3 + 4 against 7: an odd `sweep_begin` starts on the second uniform buffer
    and the other RNG buffer, and a resumed launch's first sweep finds no stage of a previous sweep to finish (its prologue
    prepares that sweep whole)."""
    K, T, burnin = 3, 897, 1
    total = sum(parts)
    nrun = total - burnin
    one = call(monkeypatch, "h", K, T, burnin, nrun)
    assert_same(one, call(monkeypatch, "p1", K, T, burnin, nrun), KEYS, equal_nan=False)
    g, base = None, 0
    for n in parts:
        last = base + n == total
        kw = dict(sweep_base=base) if last else dict(sweep_base=base, sweep_count=n)
        g = call(monkeypatch, "h", K, T, burnin, nrun, resume_state=g, **kw) if g is not None else call(monkeypatch, "h", K, T, burnin, nrun, **kw)
        d0, d1 = max(base - burnin, 0), base + n - burnin            # the draws this launch wrote
        for k in ("mu", "sig2", "pi_end", "fcast", "A"):
            assert np.array_equal(g[k][..., d0:d1], one[k][..., d0:d1]), (k, base)
        base += n
    assert np.array_equal(g["summary"], one["summary"])
    assert np.array_equal(g["x_final"], one["x_final"])
    assert np.array_equal(g["status"], one["status"])


@pytest.mark.parametrize("K", [2, 3, 4])
def test_smoothing_instantiations(hmclib, oracle, monkeypatch, K):
    """The three `SMOOTH` kernels of the six: smoothed and filtered means included."""
    T, burnin, nrun = 897, 2, 10
    Y, Tw, yreal, ids = panel(K, T)
    out = {fl: call(monkeypatch, fl, K, T, burnin, nrun, want_smooth=True, want_filter_mean=True) for fl in ("h", "p1")}
    assert_same(out["h"], out["p1"], KEYS + ("pi_smooth_mean", "pi_filter_mean", "pif_final"), equal_nan=False)
    g = out["h"]
    against_oracle(oracle, g, Y, [T, T], K, burnin, nrun, yreal, ids, want_smooth=True,
                   fields=("mu", "sig2", "A", "pi_end", "fcast", "summary", "pi_smooth_mean", "pif_final"))
    for w in range(2):
        assert np.max(np.abs(g["pi_filter_mean"][w, :T].sum(axis=1) - 1)) < 1e-12


@pytest.mark.parametrize("T", [2, 257])
def test_short_window_beside_a_long_one(hmclib, oracle, monkeypatch, T):
    """A short window beside a T = 1023 companion in one unbucketed launch: on the short window's block the ahead trip has
    no block at all and most lanes of a stage are dead."""
    K, lens = 3, [1023, T]
    Y, Tw, fut = synth.generate_panel(2, 1023, K, ragged=lens)
    yreal, ids = fut[:, [0, 11]], np.array([7, 13])
    monkeypatch.setenv("HMCG_NO_BUCKETS", "1")
    out = {}
    for fl in ("h", "p1"):
        out[fl] = g = forced_flavour_call(monkeypatch, fl, Y, Tw, K, BURNIN, NRUN, HORIZONS, yreal, window_ids=ids)
        assert g["steps_per_thread"] == 4 and g["buckets"] == 1
        assert not (g["status"] & _lib.ST_SKIPPED).any()
    assert_same(out["h"], out["p1"], KEYS, equal_nan=False)
    against_oracle(oracle, out["h"], Y, lens, K, BURNIN, NRUN, yreal, ids)
