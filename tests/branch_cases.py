"""Inputs of tests/test_gpu_branches.py, and the oracle run that tests/test_branch_coverage.py holds them to (no GPU here).

Two recipes, both aimed at the sampler's data-dependent branches, which synth.generate_panel's well separated regimes and
the argmax start never reach (the counts are in test_gpu_branches.py's docstring):

  * mixed labels (one window per kernel instantiation): synth.generate_window with state means 0.3 of a standard deviation
    apart and a uniformly random x_init.  Every state then holds a sample of the same mixture, the K posterior means differ by
    their Monte-Carlo noise only, and sortperm(mu) is close to a uniformly random permutation sweep after sweep;
  * directed (one window per branch and place): few clusters under many states, an x_init that leaves states unvisited, and
    alpha < 1 where the branch needs a gamma shape below one.  (seed, window id) of each row were found by searching with
    the oracle's branch counters; the table pins them.

A case is a Case tuple; inputs() builds its data, oracle_kwargs() / gpu_kwargs() the two calls' arguments from the same
fields, so that the CPU contract and the GPU test cannot drift apart."""
import collections

import numpy as np

from hmc_jl_amd import synth

import kernel_tables as kt
from kernel_tables import NT

HORIZONS = (1, 12)

Case = collections.namedtuple("Case", "id kind K T sig smooth env tpw burnin nrun n_samples alpha nu recipe seed window_id expect branches")
# kind: "reg" (K, L, path, flavour), "sigsmooth" (K, L), "tpw" (K, L, NT), "big" (sig, smooth, stream, K): what `expect` holds
# and which report the GPU test asserts; env: diagnostic switches the case sets; recipe: "mixed" | "sparse" | "split";
# branches: the oracle counters a directed case is listed for (mixed-label cases: empty -- they answer to the permutation shares)


# ---------------------------------------------------------------- data -------
def weak_params(K, gap=0.3):
    """K sticky regimes whose means lie `gap` standard deviations apart: no draw of mu is pinned to its label by the data."""
    A = np.full((K, K), 0.3 / (K - 1)) + (0.7 - 0.3 / (K - 1)) * np.eye(K)
    return dict(A=A, mu=gap * np.arange(K, dtype=np.float64), sig2=np.ones(K))


def two_clusters():
    """Two well separated regimes (the reference unit test's truth): with K far above two, most states stay nearly empty."""
    return synth.params_for(2)


def inputs(c):
    """Y (T,), yreal (2,), x_init (T,) int32 of a case."""
    rng = np.random.default_rng(c.seed)
    if c.recipe == "mixed":
        y = synth.generate_window(c.T + 12, c.K, 20250000 + c.seed, params=weak_params(c.K))[0]
        x0 = rng.integers(0, c.K, size=c.T)
    elif c.recipe == "sparse":                       # two clusters, every observation starts in state 0 or 1: K - 2 states start empty
        y = synth.generate_window(c.T + 12, 2, 20250000 + c.seed, params=two_clusters())[0]
        x0 = rng.integers(0, 2, size=c.T)
    elif c.recipe == "split":                        # state 0 holds the real observations, state 1 the signals, the rest nothing
        y = synth.generate_window(c.T + 12, 2, 20250000 + c.seed, params=two_clusters())[0]
        x0 = (np.arange(c.T) >= c.T - SIG_TAIL).astype(np.int64)
    else:
        raise ValueError(c.recipe)
    return np.ascontiguousarray(y[:c.T]), y[[c.T, c.T + 11]].copy(), x0.astype(np.int32)


SIG_TAIL = 30                                        # signal positions [T - 30, T); the last two are saved
KAPPA, SIGMA_SIGNAL = 0.6, 0.5


def sig_ranges(c):
    return (c.T - SIG_TAIL, c.T), (c.T - 2, c.T)


def oracle_kwargs(c, yreal, x0):
    """oracle.estimate_signals(Y, K, burnin, nrun, **these): with an empty `sig` that is the base-path run at alpha / nu."""
    kw = dict(n_samples=c.n_samples, alpha=c.alpha, nu=c.nu, horizons=HORIZONS, yreal=yreal, window_id=c.window_id, x_init=x0,
              want_smooth=c.smooth, want_filter_mean=c.smooth)
    if c.sig:
        sg, sv = sig_ranges(c)
        kw.update(sig=sg, save=sv, kappa=KAPPA, sigma_signal=SIGMA_SIGNAL)
    return kw


def gpu_kwargs(c, x0):
    """_lib.estimate_batch_host(Y[None], [T], K, burnin, nrun, HORIZONS, yreal[None], **these)."""
    kw = dict(want_state=True, window_ids=[c.window_id], x_init=x0[None, :], alpha=c.alpha, nu=c.nu, threads_per_window=c.tpw,
              want_smooth=c.smooth, want_filter_mean=c.smooth)
    if c.sig:
        sg, sv = sig_ranges(c)
        kw.update(sig_range=np.array([sg], dtype=np.int32), save_range=np.array([sv], dtype=np.int32), kappa=KAPPA,
                  sigma_signal=np.array([SIGMA_SIGNAL]), n_samples=c.n_samples, want_sample_summary=True)
    else:
        kw.update(want_corr=not c.smooth, want_smooth_draws=c.smooth)     # base runs only (plan.hpp, check_extras)
    return kw


def run_oracle(oracle, c):
    Y, yreal, x0 = inputs(c)
    return oracle.estimate_signals(Y, c.K, c.burnin, c.nrun, **oracle_kwargs(c, yreal, x0))


# ------------------------------------------------- mixed-label cases --------
# (K, T, sig, smooth) -> window id, where the default stream (window 5) misses the permutation shares on the oracle: at K = 3
# two of the six orders are 3-cycles, so about one chain in eight shows none in five kept sweeps
MIXED_OVERRIDES = {(3, 2010, False, False): 7, (3, 2010, True, False): 6, (3, 2010, False, True): 7, (3, 2010, True, True): 6,
                   (3, 4397, False, False): 6, (3, 7935, False, False): 7, (3, 2349, False, True): 6, (3, 7935, False, True): 7}


def _mixed(cid, kind, K, T, sig, smooth, env, tpw, expect):
    seed, wid = 1, MIXED_OVERRIDES.get((K, T, sig, smooth), 5)
    b, n, ns = (1, 3, 2) if sig else (2, 5, 1)       # signal paths: two chained noise samples
    a = 2.0 if sig else 1.0                          # HyperParams(opt) on the signal paths, HyperParams(Y, D) elsewhere
    return Case(cid, kind, K, T, sig, smooth, env, tpw, b, n, ns, a, a, "mixed", seed, wid, tuple(expect), ())


def reg_length(L):
    """A length only the L-steps-per-thread class takes: 37 short of its capacity (the per-variant sweep runs at 1 and 130 short)."""
    return NT * L - (1 if L > 1 else 0) - 37


def mixed_cases():
    """One window for every instantiation the coverage contract names (tests/test_variant_coverage.py), from the same lists."""
    out = []
    for (K, L, path, fl) in kt.VARIANT_CASES:
        out.append(_mixed("K%d-L%d-%s-%s" % (K, L, path, fl), "reg", K, reg_length(L), path == "sig", path == "smooth",
                          {"HMCG_FLAVOUR": fl}, 0, (K, L, path, fl)))
    for (K, L) in kt.SIGSMOOTH:
        out.append(_mixed("sigsmooth-K%d-L%d" % (K, L), "sigsmooth", K, reg_length(L), True, True, {}, 0, (K, L)))
    for (K, L, nt) in kt.OWN_THREAD_COUNT:
        out.append(_mixed("tpw-K%d-L%d-NT%d" % (K, L, nt), "tpw", K, 1000, False, False, {}, nt, (K, L, nt)))
    for (sig, sm, st, K) in kt.BIG:
        out.append(_mixed("big-%s-K%d" % (kt.form_id(sig, sm, st), K), "big", K, kt.coverage_lengths(sig, sm, st, K)[0], sig, sm,
                          {}, 0, (sig, sm, st, K)))
    return out


# ---------------------------------------------------- directed cases --------
# Where the draw code lives: the register-resident kernel (gibbs_device.hpp) in its three flavours -- attempts 0 and 1 of a
# gamma draw are prepared by shadow waves (p1, p2) or helper waves (h) --, and the LDS-resident kernel (gibbs_big.hpp) in its
# LDS and streaming forms.  K >= 5 has no register-resident row (plan.hpp: K < 5), so the LDS places run at K >= 5.
#   place: (kind, K, T of the short case, T >= 1000, env, expect builder)
def _place(place, K, T, sig):
    if place in ("p1", "p2", "h"):
        L = kt.steps_per_thread(K, T, sig)
        return "reg", {"HMCG_FLAVOUR": place}, (K, L, "sig" if sig else "base", place)
    stream = place == "stream"
    assert (kt.dyn_bytes((T + NT - 1) // NT) > kt.LDS_LIMIT) == stream and T > kt.ladder_ceiling(K, sig, False), (place, K, T)
    return "big", {}, (sig, False, stream, K)


# name, place, K, T, sig, recipe, alpha, sweeps, (seed, window id), branches the row is listed for
DIRECTED_TABLE = [
    ("small-shape", "p1", 4, 60, False, "sparse", 0.25, 8, (1, 84), ("shape_lt1", "v_rejects")),
    ("small-shape", "p2", 4, 60, False, "sparse", 0.25, 8, (1, 84), ("shape_lt1", "v_rejects")),
    ("small-shape", "h", 4, 60, False, "sparse", 0.25, 8, (1, 84), ("shape_lt1", "v_rejects")),
    ("small-shape", "lds", 6, 90, False, "sparse", 0.25, 8, (1, 84), ("shape_lt1", "v_rejects")),
    ("small-shape", "stream", 8, 7935, False, "sparse", 0.25, 6, (1, 18), ("shape_lt1", "v_rejects")),
    ("third-attempt-sig2", "p1", 4, 60, False, "sparse", 0.25, 8, (1, 35), ("gamma_3plus_sig2",)),
    ("third-attempt-sig2", "p2", 4, 60, False, "sparse", 0.25, 8, (1, 35), ("gamma_3plus_sig2",)),
    ("third-attempt-sig2", "h", 4, 60, False, "sparse", 0.25, 8, (1, 35), ("gamma_3plus_sig2",)),
    ("third-attempt-sig2", "lds", 6, 90, False, "sparse", 0.25, 8, (1, 213), ("gamma_3plus_sig2",)),
    ("third-attempt-sig2", "stream", 8, 7935, False, "sparse", 0.25, 6, (1, 204), ("gamma_3plus_sig2",)),
    ("third-attempt-A", "p1", 4, 60, False, "sparse", 0.25, 8, (1, 177), ("gamma_3plus_A",)),
    ("third-attempt-A", "p2", 4, 60, False, "sparse", 0.25, 8, (1, 177), ("gamma_3plus_A",)),
    ("third-attempt-A", "h", 4, 60, False, "sparse", 0.25, 8, (1, 177), ("gamma_3plus_A",)),
    ("third-attempt-A", "lds", 6, 90, False, "sparse", 0.25, 8, (1, 36), ("gamma_3plus_A",)),
    ("third-attempt-A", "stream", 8, 7935, False, "sparse", 0.25, 6, (1, 1), ("gamma_3plus_A",)),
    ("empty-long", "p1", 4, 1000, False, "sparse", 1.0, 3, (1, 7), ("empty_states", "x_uniform_fallbacks")),
    ("empty-long", "p2", 4, 1000, False, "sparse", 1.0, 3, (1, 7), ("empty_states", "x_uniform_fallbacks")),
    ("empty-long", "h", 4, 1000, False, "sparse", 1.0, 3, (1, 7), ("empty_states", "x_uniform_fallbacks")),
    ("empty-long", "lds", 6, 1000, False, "sparse", 1.0, 3, (1, 0), ("empty_states",)),
    ("empty-long", "stream", 8, 7935, False, "sparse", 1.0, 3, (1, 0), ("empty_states", "x_uniform_fallbacks")),
    ("one-population", "p1", 3, 200, True, "split", 2.0, 3, (1, 0), ("sig_only_states", "real_only_states")),
    ("one-population", "p2", 3, 200, True, "split", 2.0, 3, (1, 0), ("sig_only_states", "real_only_states")),
    ("one-population", "h", 3, 200, True, "split", 2.0, 3, (1, 0), ("sig_only_states", "real_only_states")),
    ("one-population", "lds", 5, 300, True, "split", 2.0, 3, (1, 0), ("sig_only_states", "real_only_states")),
    ("one-population", "stream", 5, 7935, True, "split", 2.0, 3, (1, 0), ("sig_only_states", "real_only_states")),
]


def directed_cases(table=None):
    out = []
    for (name, place, K, T, sig, recipe, alpha, sweeps, (seed, wid), branches) in (DIRECTED_TABLE if table is None else table):
        kind, env, expect = _place(place, K, T, sig)
        out.append(Case("%s-%s" % (name, place), kind, K, T, sig, False, env, 0, 0, sweeps, 2 if sig else 1, alpha, 1.0, recipe, seed, wid,
                        expect, tuple(branches)))
    return out


# ------------------------------------------------------ the conditions ------
def mixed_conditions(c, br, status):
    """What the oracle alone must show on a mixed-label case; returns the list of misses (empty: met)."""
    miss = []
    if status != 0:
        miss.append("status %d" % status)
    if 3 * br["kept_perm_sweeps"] < br["kept_sweeps"] or br["kept_sweeps"] < 1:
        miss.append("non-identity order on %d of %d kept sweeps (< 1/3)" % (br["kept_perm_sweeps"], br["kept_sweeps"]))
    if c.K >= 3 and br["kept_noninvol_sweeps"] < 1:
        miss.append("no kept sweep whose order is not its own inverse")
    return miss


def directed_conditions(c, br, status):
    miss = ["branch %s not reached" % b for b in c.branches if br[b] < 1]
    if "empty_states" in c.branches and c.T < 1000 and c.id.startswith("empty"):
        miss.append("the empty-state case must be 1000 steps or longer")
    return miss
