"""The K = 8 assembly loops (csrc/replay_asm_k8.inc, csrc/product_asm_k8.inc) against the oracle, on data that drive the
replay's eps() guard both ways at most steps.

  * the eps() guard: a label whose pif[t, s] is not > eps() takes the uniform draw.  Until the guard compared into eight
    masks, each select read the vcc of the compare right above it with no wait state, so a stale mask (the previous
    label's) could only show where pif[t, s-1] and pif[t, s] lie on opposite sides of eps().  Tight, well separated regimes
    make that happen at most steps; the test counts them on the oracle's pif_final (the last sweep's, a proxy for the earlier
    sweeps, which run the assembly loop) and requires most of T.  The state path after those sweeps must equal the oracle's;
  * emission underflow on the assembly path (the outlier case of test_gpu_parity's K = 3 status test).

Not reached here, and not reachable through the API at all: the replay's rare path (a step's total not > 0) and the
product's rescale with the largest exponent outside [1, 0x7f7].  The pdf pass scales each step's pdfs so that the largest
lies in [0.5, 1) -- or sets them all to 1 and flags the step, which is how the underflow case above is flagged -- so the
rescale branch would need an entry of A below ~1e-38 and the rare path one below ~1e-323 (A's rows are Dirichlet(counts + 1)
draws); tests/test_asm_semantics.py checks both blocks on the CPU instead.

Each case runs twice: without want_state (every sweep on the assembly replay) and with it (x_final; the last sweep runs the
C++ replay, the earlier ones the assembly loop).  The two differ only in the last sweep's replay, whose visible output is
pi_end (and the forecasts drawn from it): those must agree bit for bit.  T = 3000 is a multiple of the kernel's steps per
thread (12), 3001 is not."""
import numpy as np
import pytest

from hmc_jl_amd import _lib, synth
from oracle_parity import assert_same, assert_window_matches_oracle

pytestmark = pytest.mark.gpu
K = 8
EPS = float(np.finfo(np.float64).eps)
LENS = (3000, 3001)


def regimes(T, seed, stay=0.97, sd=0.05, gap=1.0):
    """eight sticky regimes at 0, 1, ..., 7 with sd 0.05: the filter is sure of the current one, the others sit at 0"""
    rng = np.random.default_rng(seed)
    x = np.empty(T, dtype=np.int64)
    x[0] = rng.integers(K)
    for t in range(1, T):
        x[t] = x[t - 1] if rng.random() < stay else rng.integers(K)
    return gap * x + sd * rng.standard_normal(T)


def run_both(oracle, Y, Tw, burnin, nrun, x_init=None):
    """the run without want_state, the run with it, and the oracle per window: parity, and the two runs' draws equal"""
    kw = dict(x_init=x_init) if x_init is not None else {}
    g = _lib.estimate_batch_host(Y, Tw, K, burnin, nrun, (12,), None, **kw)
    gs = _lib.estimate_batch_host(Y, Tw, K, burnin, nrun, (12,), None, want_state=True, **kw)
    draws = ("mu", "sig2", "A", "pi_end", "fcast", "summary")
    assert_same(g, gs, draws + ("status",))
    outs = []
    for w in range(Y.shape[0]):
        T = int(Tw[w])
        o = oracle.estimate_window(Y[w, :T], K, burnin, nrun, (12,), None, window_id=w,
                                   x_init=None if x_init is None else x_init[w, :T])
        # the draws of the run without want_state (equal to the other's, above), the states and the last filter of the one with it
        assert_window_matches_oracle(gs, w, T, o, fields=("mu", "sig2", "A", "pi_end", "pif_final"), status0=False)
        outs.append(o)
    return g, outs


def test_eps_guard_straddling_steps(hmclib, oracle):
    W = len(LENS)
    Y = np.zeros((W, max(LENS)))
    for w, T in enumerate(LENS):
        Y[w, :T] = regimes(T, 7 + w)
    Tw = np.array(LENS, dtype=np.int32)
    g, outs = run_both(oracle, Y, Tw, 2, 6)
    assert (g["status"] == 0).all()
    for w, o in enumerate(outs):
        low = o["pif_final"] <= EPS                                   # (T, K), the sampler's own label order
        straddle = (low[:, 1:] != low[:, :-1]).any(axis=1)
        share = float(straddle.mean())
        print("T=%d: eps()-straddling steps %.3f of T" % (LENS[w], share))
        assert share > 0.5, share                                     # measured 0.99 and 1.00 on these data (oracle)


def outlier_case(T):
    """teacher-forced into state 0: a 1e6 outlier at step 1500 of an otherwise ordinary K = 8 panel row"""
    Y, _, _ = synth.generate_panel(1, T, K)
    Y[0, 1500] = 1e6
    return Y, np.array([T], dtype=np.int32), np.zeros((1, T), dtype=np.int32)


@pytest.mark.parametrize("T", LENS)
def test_emission_underflow_on_the_assembly_path(hmclib, oracle, T):
    """sd_0 ~ 1e6 / sqrt(T) puts the single outlier ~55 sd out of state 0 and the empty states' prior draws further: every pdf of
    that step underflows.  The pdf pass flags the window and hands that step f = 1 for every state (so the replay's rare path
    is not taken: the step's total is 1); the flag and the rest of the window agree with the oracle"""
    Y, Tw, x0 = outlier_case(T)
    g, (o,) = run_both(oracle, Y, Tw, 0, 1, x_init=x0)
    assert o["status"] & _lib.ST_EMIS_UNDERFLOW and g["status"][0] & _lib.ST_EMIS_UNDERFLOW
    assert np.isfinite(g["mu"]).all() and np.isfinite(g["pi_end"]).all()
