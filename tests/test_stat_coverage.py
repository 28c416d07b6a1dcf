"""The per-instantiation contract of the draw-statistic kernels, checked without a GPU: every instantiation of the eight
templated statistic kernels in the built library -- predictive_cdf_kernel<K>, fan_eval_kernel<K>, score_comp_kernel<K>,
score_pair_kernel<NH>, mixmoments_kernel<K, NHC>, bias_moments_kernel<K>, ergodic_kernel<K>, draw_moments_kernel<PPT> -- is
launched by a case of the GPU suite's reference tests, and no case launches a kernel that is not compiled.  The sampler's
contract is tests/test_variant_coverage.py; cases_of and the symbol reader are shared with it (tests/kernel_tables.py).

Compiled set: the kernel handles of libhmcgibbs.so's dynamic symbol table (nm -D; the statistic kernels' handles are there,
beside their __device_stub__ twins), with the expected count of each kernel asserted, so that a pattern which silently drops a
symbol fails.  Named set: the parametrize lists of test_device_entry_against_reference in the five feature modules (the score
module's is score_cases.GPU_CASES), ergodic_cases.KS and corr_cases.accumulation_cases(), each case mapped to what its call
launches by the launch rules parsed from the sources (kernel_tables.stat_launch_rules: HMCG_SWITCH_K, score.hip's switch
(a.n_h), mixmoments.hip's a.n_h <= 2; the pairs-per-thread rule of moments.hip is held to its source by
tests/test_corr_cases.py).  A changed launch rule changes the named set and fails here.

The K = 4..7 cases are held to what they were added for: every such K meets every option of its table's deal, the sizes on
both sides of each tile edge, both NHC builds, the largest LDS tile; bias meets every value of items(K) mod 4 and both sides of
its unroll switch (both parsed from bias.hip); and each of these cases has, from its reference module alone, a finite
reference and a positive bound, the long-double score reference inside score_cases.PAIR_BUDGET."""
import numpy as np
import pytest

import bias_cases as bc
import corr_cases as cc
import ergodic_cases as ec
import fan_cases as fc
import kernel_tables as kt
import mixmoments_cases as mc
import predictive_cases as pc
import score_cases as sc
import test_gpu_bias as bias
import test_gpu_corr_kernels as corr
import test_gpu_ergodic as erg
import test_gpu_fan as fan
import test_gpu_mixmoments as mix
import test_gpu_predictive as pred
import test_gpu_score as score
import test_gpu_stat_omega as omega

NEW_KS = (4, 5, 6, 7)
EXPECTED = {"predictive_cdf_kernel": 7, "fan_eval_kernel": 7, "score_comp_kernel": 7, "score_pair_kernel": 8, "mixmoments_kernel": 14,
            "bias_moments_kernel": 7, "ergodic_kernel": 7, "draw_moments_kernel": len(set(cc.PPT_OF_K.values()))}
# The instantiations no test launched before the K = 4..7 cases: they must be in the named map, whatever else changes.
ONCE_UNRUN = ([(k, (K,)) for k in ("predictive_cdf_kernel", "fan_eval_kernel", "score_comp_kernel", "bias_moments_kernel") for K in NEW_KS]
              + [("score_pair_kernel", (n,)) for n in (5, 6, 7)] + [("mixmoments_kernel", (K, n)) for K in NEW_KS for n in (2, 8)])


def fmt(inst):
    name, args = inst
    return "%s<%s>" % (name, ", ".join(str(a) for a in args))


def tables():
    """The case lists of the five feature modules, as the GPU suite runs them."""
    return {"predictive": kt.cases_of(pred.test_device_entry_against_reference), "fan": kt.cases_of(fan.test_device_entry_against_reference),
            "score": kt.cases_of(score.test_device_entry_against_reference), "mixmoments": kt.cases_of(mix.test_device_entry_against_reference),
            "bias": kt.cases_of(bias.test_device_entry_against_reference)}


def named_instantiations():
    """{(kernel, template arguments): the first case that launches it}, by the launch rules of the sources."""
    rules = kt.stat_launch_rules()
    by_k, pair, (limit, small, large) = rules["K"], rules["pair"], rules["nhc"]
    t = tables()
    assert t["score"] == sc.GPU_CASES
    named = {}

    def name(kernel, args, case):
        named.setdefault((kernel, tuple(args)), case)
    for c in t["predictive"]:
        name("predictive_cdf_kernel", (by_k.get(c[0], -1),), "test_gpu_predictive %s" % (c,))
    for c in t["fan"]:
        name("fan_eval_kernel", (by_k.get(c[0], -1),), "test_gpu_fan %s" % (c,))
    for c in t["score"]:
        K, hz = c[0], c[5]
        name("score_comp_kernel", (by_k.get(K, -1),), "score_cases.GPU_CASES %s" % (c,))
        name("score_pair_kernel", (pair.get(len(hz), -1),), "score_cases.GPU_CASES %s" % (c,))
    for c in t["mixmoments"]:
        K, hz = c[0], c[3]
        name("mixmoments_kernel", (by_k.get(K, -1), small if len(hz) <= limit else large), "test_gpu_mixmoments %s" % (c,))
    for c in t["bias"]:
        name("bias_moments_kernel", (by_k.get(c[0], -1),), "test_gpu_bias %s" % (c,))
    assert kt.cases_of(erg.test_columns_equal_the_restatement_bit_for_bit, "K") == list(ec.KS)
    for K in ec.KS:
        name("ergodic_kernel", (by_k.get(K, -1),), "ergodic_cases.KS %d" % K)
    assert kt.cases_of(corr.test_accumulation_and_finalisation) == cc.accumulation_cases()
    for c in cc.accumulation_cases():
        name("draw_moments_kernel", (cc.PPT_OF_K[c[0]],), "corr_cases.accumulation_cases %s" % (c,))
    return named


def test_compiled_set_is_read_whole():
    """7, 7, 7, 8, 14, 7, 7 and corr_cases' PPT list: what HMCG_SWITCH_K, the switch on n_h and the two NHC builds must give."""
    lib = kt.stat_instantiations()
    assert {k: len(v) for k, v in lib.items()} == EXPECTED, {k: len(v) for k, v in lib.items()}
    for k, v in lib.items():
        assert len(set(v)) == len(v), k
    rules = kt.stat_launch_rules()
    ks = sorted(rules["K"])
    assert ks == list(range(2, 9)) and all(rules["K"][K] == K for K in ks)
    maxh = kt.header_int("HMCG_MAXH")
    assert sorted(rules["pair"]) == list(range(1, maxh + 1)) and all(rules["pair"][n] == n for n in rules["pair"])
    assert rules["nhc"] == (2, 2, maxh)
    for k in ("predictive_cdf_kernel", "fan_eval_kernel", "score_comp_kernel", "bias_moments_kernel", "ergodic_kernel"):
        assert lib[k] == [(K,) for K in ks], k
    assert lib["score_pair_kernel"] == [(n,) for n in range(1, maxh + 1)]
    assert lib["mixmoments_kernel"] == sorted((K, n) for K in ks for n in (rules["nhc"][1], rules["nhc"][2]))
    assert lib["draw_moments_kernel"] == sorted((p,) for p in set(cc.PPT_OF_K.values()))


def test_every_statistic_instantiation_is_launched_by_a_case():
    lib = {(k, a) for k, v in kt.stat_instantiations().items() for a in v}
    named = named_instantiations()
    missing = sorted(lib - set(named))
    assert not missing, "compiled, but no reference case launches it: " + "; ".join(fmt(i) for i in missing)
    extra = sorted(set(named) - lib)
    assert not extra, "a case launches a kernel that is not compiled: " + "; ".join("%s -> %s" % (named[i], fmt(i)) for i in extra)
    gone = [i for i in ONCE_UNRUN if i not in named]
    assert len(ONCE_UNRUN) == 27 and not gone, "no case launches " + "; ".join(fmt(i) for i in gone)


def test_omega_bits_are_compared_at_every_k():
    assert sorted(kt.cases_of(omega.test_one_draw_gives_the_same_omega_sum_in_all_three_features, "K")) == sorted(kt.stat_launch_rules()["K"])


def test_device_panel_cases_feed_the_k5_kernels_with_the_samplers_own_draws():
    """(5, 300, 200) beside the K = 3 and K = 8 panels of every feature.  The variant tables hold no register-resident row above
    K = 4, so the K = 5 panel's draws come from the LDS-resident kernel, as the K = 8 panel's do: the case stands for the K = 5
    statistic kernels on draws the sampler made, not for another sampler form."""
    assert kt.ladder_ceiling(5, False, False) == 0 and (False, False, False, 5) in kt.BIG
    tests = (pred.test_device_panel_predictive_cdf, fan.test_device_panel_fan, score.test_device_panel_scores,
             mix.test_device_panel_mixture_moments, bias.test_device_panel_bias_moments)
    for t in tests:
        cases = kt.cases_of(t)
        assert (3, 200, 700) in cases and (5, 300, 200) in cases, t.__name__


def _met(cases, K, col):
    return {c[col] for c in cases if c[0] == K}


def test_new_k_cases_meet_every_option_and_edge():
    """What the K = 4..7 cases were added for, per table: deleting a case that alone carries one of these fails here."""
    t = tables()
    H8p = pred.H8
    for K in NEW_KS:
        # predictive (K, nd, G, W, horizons, pad, round5)
        p = t["predictive"]
        assert _met(p, K, 1) >= {1, 65, 1025} and _met(p, K, 2) >= {1, 65} and _met(p, K, 4) >= {(0,), (0, 1, 12), H8p}, K
        assert _met(p, K, 5) == {0, 5} and _met(p, K, 6) == {True, False}, K
        assert (K, 65, 65) in {c[:3] for c in p if c[4] == H8p}, K                      # the largest tile of this K
        # fan (K, nd, W, horizons, probs, rounds, pad, round5)
        f = t["fan"]
        assert _met(f, K, 1) >= {1, 65, 1025} and _met(f, K, 3) >= {(0,), (0, 1, 12)} and _met(f, K, 5) >= {1, 2}, K
        assert _met(f, K, 4) == {fc.PROBS16[7:8], fc.PROBS5, fc.PROBS16} and _met(f, K, 6) == {0, 5} and _met(f, K, 7) == {True, False}, K
        # score (K, n_u, stride, pad, round5, horizons, W)
        s = t["score"]
        assert _met(s, K, 1) == set(sc.used_counts(K)), K
        assert {len(h) for h in _met(s, K, 5)} == {2, 4, 5, 6, 7} and _met(s, K, 2) == {1, 2, 3} and _met(s, K, 3) == {0, 5}, K
        assert _met(s, K, 4) == {True, False} and _met(s, K, 6) == {1, 3}, K
        # mixmoments (K, nd, W, hz, pad, round5)
        m = t["mixmoments"]
        assert _met(m, K, 1) >= {1, 2, 65, 257, 1025} and _met(m, K, 3) == set(mix.HSETS) and _met(m, K, 2) == {1, 3}, K
        assert _met(m, K, 4) == {0, 5} and _met(m, K, 5) == {True, False}, K
        # bias (K, nd, W, horizon, pad, round5, H)
        b = t["bias"]
        assert _met(b, K, 1) >= {2, 65, 257, 1025, 2065} and _met(b, K, 3) == {0, 12} and _met(b, K, 6) == {0, 1}, K
        assert _met(b, K, 4) == {0, 5} and _met(b, K, 5) == {True, False}, K
    # the largest tile of all the K below 8 needs the attribute call: 60 928 B at K = 7, eight horizons, with A
    lds = lambda K, n_h, with_A: 8 * 64 * (2 * K + n_h * K + (K * K if with_A else 0))          # mixture_tile.hpp, mixture_lds_bytes
    assert lds(7, 8, True) == 60928 > 48 * 1024 and lds(8, 8, True) == 73728                 # 73.7 KB: the K = 8 case's own figure
    # a draw's components straddle the pair kernel's 256-component tile edge at K = 5, 6, 7
    for K in (5, 6, 7):
        n = sc.TP // K
        assert n * K < sc.TP < (n + 1) * K and {n, n + 1} <= _met(t["score"], K, 1), K
    assert all(sc.pair_cost(c[0], c[1], c[6]) <= sc.PAIR_BUDGET for c in t["score"])
    assert sc.PAIR_BUDGET == max(sc.pair_cost(c[0], c[1], c[6]) for c in t["score"] if c[0] not in NEW_KS)
    assert sc.pair_cost(sc.DEFAULT_CASE[0], sc.thinning(sc.DEFAULT_CASE[1], 0)[1], 1) <= sc.PAIR_BUDGET


def test_bias_cases_meet_every_item_remainder_and_both_unroll_paths():
    """The items are dealt over BIAS_NW waves with the tail cut by `if constexpr`: every remainder of items(K) mod BIAS_NW has a
    case; K <= unroll_max runs the unrolled sub-tiles and K above it the rolled loop: the two K at the switch have cases."""
    cst = kt.bias_constants()
    items, NW, top = cst["items"], cst["waves"], cst["unroll_max"]
    assert NW == 4 and [items(K) for K in (2, 3, 5, 8)] == [15, 28, 66, 153]          # K (2K + 1) + 2K + 1
    from hmc_jl_amd import _lib
    assert all(_lib.bias_stride(K) == 2 + 2 * K + 4 * K * K for K in range(2, 9))
    ks = {c[0] for c in tables()["bias"]}
    rem = {}
    for K in sorted(ks):
        rem.setdefault(items(K) % NW, K)
    assert sorted(rem) == list(range(NW)), "no bias case with items mod %d in %s" % (NW, sorted(set(range(NW)) - set(rem)))
    assert 2 <= top < 8 and {top, top + 1} <= ks, "no bias case at K = %d / %d, the two sides of the unroll switch" % (top, top + 1)
    assert {items(K) % NW for K in NEW_KS} == {1, 2, 3, 0}


# ---- the references of the new cases, from the reference modules alone ----
def _new(name):
    return [c for c in tables()[name] if c[0] in NEW_KS]


@pytest.mark.parametrize("K,nd,G,W,horizons,pad,round5", _new("predictive"))
def test_new_predictive_cases_have_a_finite_reference(K, nd, G, W, horizons, pad, round5):
    mu, sig2, pi, A = pc.make_draws(1000 * K + nd + G, W, K, nd, pad, max(horizons) > 0)
    exp = pc.reference(mu, sig2, pi, A, pc.make_grid(G), horizons, round5, nd)
    assert exp.shape == (W, len(horizons), G) and np.isfinite(exp).all() and (exp >= 0.0).all() and (exp <= 1.0 + 1e-3).all()
    assert 0.0 < pc.tolerance(nd, K, max(horizons)) < 1e-12


@pytest.mark.parametrize("K,nd,W,horizons,probs,rounds,pad,round5", _new("fan"))
def test_new_fan_cases_have_a_finite_reference(K, nd, W, horizons, probs, rounds, pad, round5):
    mu, sig2, pi, A = fc.make_draws(2000 * K + nd + len(probs), W, K, nd, pad, max(horizons) > 0, 1.0 if nd % 2 else 4.0)
    out, rng, flag = fc.reference(mu, sig2, pi, A, probs, horizons, rounds, round5, nd)
    assert np.isfinite(rng).all() and (rng[:, 0] < rng[:, 1]).all() and not (flag & fc.NAN_).any() and np.isfinite(out).all()
    assert (out[..., 1] <= out[..., 0]).all() and (out[..., 0] <= out[..., 2]).all()
    assert 0.0 < fc.tolF(nd, K, horizons) < 1e-12


@pytest.mark.parametrize("K,n_u,stride,pad,round5,horizons,W", _new("score"))
def test_new_score_cases_have_a_finite_reference(K, n_u, stride, pad, round5, horizons, W):
    nd = sc.nd_of(n_u, stride)
    assert sc.thinning(nd, stride) == (stride, n_u) and sc.pair_cost(K, n_u, W) <= sc.PAIR_BUDGET
    mu, sig2, pi, A = fc.make_draws(3000 * K + n_u, W, K, nd, pad, max(horizons) > 0, 1.0 if n_u % 2 else 4.0)
    y = sc.make_yreal(mu, sig2, len(horizons), nd, n_u + K)
    ref, bound = sc.reference(mu, sig2, pi, A, y, horizons, stride, round5, nd)
    unknown = np.isnan(y.T)
    assert np.isfinite(ref[..., 2]).all() and np.array_equal(np.isnan(ref[..., 0]), unknown) and np.array_equal(np.isnan(ref[..., 3]), unknown)
    ok = np.isfinite(ref)
    far = ok & (ref == 0.0)                                   # pit and pdf 40 standard deviations out are exactly 0
    assert (bound[ok & ~far] > 0.0).all() and np.isfinite(bound[ok]).all()
    assert (bound[..., 3][~unknown] > 0.0).all() and ((bound[..., 2] > 0.0).all() if n_u > 1 else True)


@pytest.mark.parametrize("K,nd,W,hz,pad,round5", _new("mixmoments"))
def test_new_mixmoments_cases_have_a_finite_reference(K, nd, W, hz, pad, round5):
    mu, sig2, pi, A = mc.make_draws(1000 * K + nd + 31 * len(hz), W, K, nd, pad, any(h > 0 for h in hz))
    ref = mc.reference(mu, sig2, pi, A, hz, round5, nd)
    tol = mc.tolerance(ref, nd, K, hz)
    for k in mc.FIELDS:
        assert np.isfinite(ref[k].astype(np.float64)).all() and np.isfinite(tol[k]).all() and (tol[k] > 0.0).all(), k


@pytest.mark.parametrize("K,nd,W,horizon,pad,round5,H", _new("bias"))
def test_new_bias_cases_have_a_finite_reference(K, nd, W, horizon, pad, round5, H):
    mu, pi, A, fcast = bc.make_draws(1000 * K + nd + 31 * horizon, W, K, nd, pad, horizon > 0, H)
    ref = bc.reference(mu, pi, A, fcast, horizon, round5, nd)
    tol = bc.tolerance(ref, nd, K, horizon)
    for k in ("uncbias", "mean", "cov") + (("totalbias",) if H else ()):
        assert np.isfinite(ref[k].astype(np.float64)).all() and np.isfinite(tol[k]).all() and (tol[k] > 0.0).all(), k
    assert H > 0 or np.isnan(ref["totalbias"].astype(np.float64)).all()
