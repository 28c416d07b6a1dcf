"""The forward filter's cross-wave prefix of the K <= 4 sweep (gibbs_device.hpp, between barriers Bc and Bd): wave 0
publishes the vector rho' W_0 instead of its total W_0, a wave w >= 1 starts from that vector and multiplies by the totals
of waves 1..w-1 on a straight-line path of its own, and every lane multiplies the vector by its own inclusive product before
the result moves one lane up (lane 0 keeps the vector).

What can go wrong shows where the data ends on or next to a wave boundary, and a class's own length range (769..1024 for
four steps per thread) never puts it there: the calls below are unbucketed (HMCG_NO_BUCKETS), so that short windows run on
the long window's kernel.  Per steps-per-thread class L (256 threads, wave = 64 L steps) one ragged call with the windows

    256 L, 256 L - 1          the longest window (it selects the class), and one step less
    64 L, 128 L, 192 L        the data ends exactly on a wave boundary: the last live wave's successor holds padding only
    64 L + 1, ... 192 L + 1   the first lane of a wave holds the last real step: lane 0 keeps the incoming vector
    L + 1                     only lanes 0 and 1 of wave 0 are live
    2                         the shortest window the entry accepts

The same windows move the backward phase's lane predicates (which slot holds the last step, which slots are padding, the
lane's row), rebuilt every sweep from per-lane values instead of being kept as masks, through every position in a thread, a
row and a wave.

The calls: every class compiled for K = 2, 3, 4 and every flavour (h, p1, p2: all three exist for every base class), 2 + 6 sweeps;
the two-wave (128 threads, L = 8) and eight-wave (512 threads, L = 2: the only six-product chain) rows of K = 3 with the
boundaries at 64 L j, j < NW; and the smoothing form of K = 3, L = 4, whose backward chain reads the totals of waves 1.. and
must not miss W_0.  Asserted: status 0, the state path equal to the oracle's, every float output within 1e-9 relative to
1 + |x| (the suite's tolerance), and the flavours equal to each other bit for bit."""
import numpy as np
import pytest

from hmc_jl_amd import synth
from kernel_tables import register_classes
from oracle_parity import assert_batch_matches_oracle, assert_same, assert_window_matches_oracle, forced_flavour_call

pytestmark = pytest.mark.gpu
BURNIN, NRUN, HORIZONS = 2, 6, (1, 12)
FLOATS = ("mu", "sig2", "A", "pi_end", "fcast", "summary")
KEYS = FLOATS + ("x_final", "status")
FLAVOURS = ("h", "p1", "p2")
# the steps-per-thread classes of the base path's 256-thread rows (csrc/variants_k2|k3|mid|k3_l16|k4.hip), from the parsed tables
CLASSES = {K: tuple(register_classes(K, False, False)) for K in (2, 3, 4)}
CASES = [(K, L) for K in (2, 3, 4) for L in CLASSES[K]]
WIDE = [(128, 8), (512, 2)]                     # (threads per window, L): HMCG_V(3, 8, 128, ...) and HMCG_V(3, 2, 512, ...)


def lengths(L, nw=4):
    edge = [64 * L * j for j in range(1, nw)]
    return [64 * L * nw, 64 * L * nw - 1] + edge + [e + 1 for e in edge] + [L + 1, 2]


_panels, _runs, _oracle = {}, {}, {}


def panel(K, L, nw=4):
    if (K, L, nw) not in _panels:
        lens = lengths(L, nw)
        Y, Tw, fut = synth.generate_panel(len(lens), max(lens), K, ragged=lens)
        _panels[K, L, nw] = (Y, Tw, np.ascontiguousarray(fut[:, [0, 11]]))
    return _panels[K, L, nw]


def run(monkeypatch, flavour, K, L, nt=0, **kw):
    """The ragged call of class L in one unbucketed launch under the forced flavour (None: the row's own)."""
    key = (flavour, K, L, nt) + tuple(sorted(kw))
    if key not in _runs:
        monkeypatch.setenv("HMCG_NO_BUCKETS", "1")
        Y, Tw, yreal = panel(K, L, nt // 64 if nt else 4)
        g = forced_flavour_call(monkeypatch, flavour, Y, Tw, K, BURNIN, NRUN, HORIZONS, yreal, threads_per_window=nt, **kw)
        assert g["steps_per_thread"] == L and g["threads_per_window"] == (nt or 256) and g["buckets"] == 1
        _runs[key] = g
    return _runs[key]


def reference(oracle, K, L, nw=4):
    """The oracle's run of the panel, on the CPU; it must accept every window by itself before anything goes to the GPU."""
    if (K, L, nw) not in _oracle:
        Y, Tw, yreal = panel(K, L, nw)
        _oracle[K, L, nw] = oracle.estimate_batch(Y, Tw, K, BURNIN, NRUN, HORIZONS, yreal, want_state=True)
    assert (_oracle[K, L, nw]["status"] == 0).all(), "the oracle itself flags a window: replace it"
    return _oracle[K, L, nw]


@pytest.mark.parametrize("K,L", CASES, ids=["K%d-L%d" % c for c in CASES])
def test_wave_edges_against_oracle(hmclib, oracle, monkeypatch, K, L):
    o = reference(oracle, K, L)
    assert_batch_matches_oracle(run(monkeypatch, "h", K, L), o, FLOATS)


@pytest.mark.parametrize("K,L", CASES, ids=["K%d-L%d" % c for c in CASES])
def test_wave_edges_flavours_equal_bit_for_bit(hmclib, oracle, monkeypatch, K, L):
    reference(oracle, K, L)
    h = run(monkeypatch, "h", K, L)
    assert_same(h, run(monkeypatch, "p1", K, L), KEYS, equal_nan=False)
    assert_same(h, run(monkeypatch, "p2", K, L), KEYS, equal_nan=False)


@pytest.mark.parametrize("nt,L", WIDE, ids=["2-waves", "8-waves"])
def test_two_and_eight_waves(hmclib, oracle, monkeypatch, nt, L):
    """No product at all (two waves: wave 1 takes the vector as it is) and the six-product chain (eight waves)."""
    o = reference(oracle, 3, L, nt // 64)
    assert_batch_matches_oracle(run(monkeypatch, None, 3, L, nt), o, FLOATS)


def test_smoothing_reads_the_later_totals_only(hmclib, oracle, monkeypatch):
    """K = 3, L = 4 with extras.pi_smooth_mean: the backward chain multiplies by the totals of waves 1.. -- slot 0 now holds a
    vector."""
    K, L = 3, 4
    Y, Tw, yreal = panel(K, L)
    ref = reference(oracle, K, L)
    smooth = [oracle.estimate_window(Y[w, :T], K, BURNIN, NRUN, HORIZONS, yreal[w], window_id=w, want_smooth=True) for w, T in enumerate(Tw)]
    assert all(o["status"] == 0 for o in smooth)
    out = {fl: run(monkeypatch, fl, K, L, want_smooth=True) for fl in FLAVOURS}
    assert_same(out["h"], out["p1"], KEYS + ("pi_smooth_mean",), equal_nan=False)
    assert_same(out["h"], out["p2"], KEYS + ("pi_smooth_mean",), equal_nan=False)
    g = out["h"]
    assert_batch_matches_oracle(g, ref, FLOATS)
    for w, T in enumerate(Tw):
        assert_window_matches_oracle(g, w, T, smooth[w], fields=("pi_smooth_mean",))
