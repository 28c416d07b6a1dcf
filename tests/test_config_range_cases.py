"""The contract of tests/test_gpu_config_range.py, checked without a GPU (as test_variant_coverage.py and
test_branch_coverage.py hold their tables).

tests/config_range_cases.py is the one table both modules read.  Here:
  * its coverage: every H in 0..8 on the register-resident and the LDS-resident route, H = 8 on every route and path, every
    blend_mask bit, the horizons 25 | 26 | 27 together, a 64-bit seed and a window id >= 2^31 per route, the wrapped
    window_base, the other priors, one unknown yreal column per H = 8 case;
  * each case's lengths and switches select the route it claims, by the parsed variant tables;
  * the oracle alone on every case: status 0; its forecasts within 1e-11 (relative to 1 + |x|) of pi_end' A^h mu recomputed
    in numpy.longdouble from its own draws -- measured: 1.6e-13 for horizons up to 5000 at K = 2..8 when the table was drawn
    up, 2.4e-13 at most over the table as it stands; the margin covers other seeds --; a
    blended slot's columns do not depend on its `horizons` entry.  This keeps the GPU test's reference honest.
What this does not show: that the GPU agrees -- test_gpu_config_range.py's business."""
import numpy as np
import pytest

import config_range_cases as cr
import kernel_tables as kt
import test_gpu_config_range as gpu
import test_variant_coverage as cov

CASES = cr.CASES
ORACLE_FORECAST_BOUND = 1e-11


def of(route=None, path=None):
    return [c for c in CASES if route in (None, c.route) and path in (None, c.path)]


def test_the_gpu_module_runs_this_table():
    assert list(cov.cases_of(gpu.test_case_against_oracle)) == CASES
    assert list(cov.cases_of(gpu.test_forecasts_from_the_calls_own_draws)) == CASES
    assert list(cov.cases_of(gpu.test_summaries_from_the_calls_own_draws)) == CASES
    assert len(cr.BY_ID) == len(CASES)
    h8 = [c for c in CASES if len(c.horizons) == 8]
    assert list(cov.cases_of(gpu.test_chunked_run_equals_one_launch)) == h8
    assert list(cov.cases_of(gpu.test_device_entry_equals_host_entry)) == [c for c in h8 if c.route in ("register", "lds")]
    assert list(cov.cases_of(gpu.test_three_devices_equal_one)) == [c for c in h8 if len(c.lens) >= 3]
    assert list(cov.cases_of(gpu.test_wrapped_window_base_equals_explicit_ids)) == [c for c in CASES if c.window_base]
    assert list(cov.cases_of(gpu.test_cut_chain_equals_one_launch)) == [c for c in CASES if c.split]


def test_horizon_counts():
    for route in ("register", "lds"):
        assert {len(c.horizons) for c in of(route)} >= set(range(9)), route
    for route in cr.ROUTES:
        assert any(len(c.horizons) == 8 for c in of(route)), route
    for route in ("register", "lds"):
        for path in cr.PATHS:
            assert any(len(c.horizons) == 8 for c in of(route, path)), (route, path)
    for c in CASES:
        H = len(c.horizons)
        assert H <= 8 and all(0 <= h <= cr.MAX_HORIZON or (h == cr.JUNK_HORIZON and k in c.blend) for k, h in enumerate(c.horizons)), c.id
        assert c.horizons in (cr.FULL[:H], cr.REVERSED) or c.path == "tail", c.id
    assert any(c.horizons == cr.REVERSED for c in of("register")) and any(c.horizons == cr.REVERSED for c in of("lds"))
    assert cr.FULL[5] == cr.FULL[6]                                         # the repeated horizon


def test_horizons_25_26_27_occur_together():
    for route in cr.ROUTES:
        assert any({25, 26, 27} <= set(c.horizons) for c in of(route)), route


def test_blend_bits():
    tails = of(path="tail")
    assert {b for c in tails for b in c.blend} == set(range(8))
    for route in ("register", "lds"):
        mine = of(route, "tail")
        assert any(c.blend == (5,) for c in mine) and any(c.blend == (3, 7) for c in mine), route
        assert any(all(c.horizons[b] == cr.JUNK_HORIZON for b in c.blend) for c in mine), route
    for c in tails:
        assert len(c.horizons) == 8 and c.sigLen > 0 and all(b < 8 for b in c.blend), c.id
        assert any(k not in c.blend for k in range(8)), c.id
        assert min(c.lens) - 1 - c.sigLen >= 1, c.id                      # end_pos inside the window
    assert {(c.K, c.lens[0], c.sigLen) for c in tails} == {(3, 140, 12), (8, 200, 48)}
    assert all(not c.blend for c in CASES if c.path != "tail")


def test_seeds_and_window_ids():
    for route in cr.ROUTES:
        mine = of(route)
        assert any(c.seed == cr.SEED_GOLDEN for c in mine), route
        assert any(c.seed == cr.SEED_HIGH_WORD for c in mine), route
        assert any(c.seed >> 32 for c in mine) and any(max(cr.ids_of(c)) >= 2 ** 31 for c in mine), route
        assert any(c.window_ids == cr.TOP_IDS[:len(c.lens)] for c in mine), route
        wrapped = [c for c in mine if c.window_base == cr.WRAP_BASE and c.window_ids is None]
        assert wrapped and all(cr.ids_of(c) == [0xFFFFFFFE, 0xFFFFFFFF, 0] for c in wrapped), route
    assert cr.SEED_HIGH_WORD & 0xFFFFFFFF == cr.SEED_DEFAULT == 1234


def test_priors_and_unknown_realised_values():
    for route in ("register", "lds"):
        assert any((c.alpha, c.nu) == (3.5, 0.25) for c in of(route, "base")), route
    assert all((c.alpha, c.nu) == (2.0, 2.0) for c in CASES if c.path != "base")
    h8 = [c for c in CASES if len(c.horizons) == 8]
    assert all(c.nan_col is not None and 0 <= c.nan_col < 8 for c in h8)
    assert all(a.nan_col != b.nan_col for a, b in zip(h8, h8[1:])) and {c.nan_col for c in h8} == set(range(8))
    assert all(c.nan_col is None for c in CASES if len(c.horizons) < 8)


def test_sweeps_and_splits():
    splits = [c for c in CASES if c.split]
    assert all(c.sweeps == (cr.SPLIT_SWEEPS if c.split else cr.SWEEPS) for c in CASES)
    assert {(c.route, c.path) for c in splits} >= {("register", "base"), ("lds", "base")} and any(c.path == "sig" for c in splits)
    assert all(len(c.horizons) == 8 for c in splits)
    burnin, nrun = cr.SPLIT_SWEEPS
    cuts = [s for (s,) in cr.SPLIT_CUTS]
    assert any(0 < s < burnin for s in cuts) and burnin in cuts and any(burnin < s < burnin + nrun for s in cuts)


def test_shapes_are_the_issues():
    reg = {(c.K, dict(c.env).get("HMCG_FLAVOUR")) for c in of("register", "base") if c.lens == (200, 65, 2)}
    assert reg >= {(K, f) for K in (2, 3, 4) for f in ("p1", "p2", "h")}
    assert {(c.K, c.tpw, c.lens) for c in of("tpw")} == {(3, 128, (1000,) * 3), (3, 512, (1000,) * 3)}
    lds = {(c.K, c.lens) for c in of("lds", "base")}
    assert lds >= {(5, (130, 64, 2)), (7, (130,)), (8, (300, 65)), (3, (200,))}
    assert {(c.K, c.lens[0]) for c in of("stream")} == {(3, 300), (8, 300)}
    assert {(c.route, c.K, c.lens) for c in of(path="sig") if not c.split} == {("register", 3, (140, 133)), ("lds", 6, (150,))}


def test_each_case_selects_the_route_it_claims():
    for c in CASES:
        route, L = cr.planned_route(c)
        assert route == c.route, (c.id, route)
        if c.route in ("lds", "stream"):
            assert L == (max(c.lens) + 255) // 256, c.id
        if c.route == "register":
            assert c.K <= 4 and max(c.lens) <= kt.ladder_ceiling(c.K, cr.is_sig(c), False), c.id
        if c.route == "lds":
            assert c.K >= 5 or dict(c.env).get("HMCG_FORCE_BIG"), c.id


_ORACLE = {}


def oracle_runs(oracle, c):
    """The oracle on every window of the case, once per session."""
    if c.id not in _ORACLE:
        Y, Tw, yreal = cr.inputs(c)
        _ORACLE[c.id] = (Y, Tw, yreal, [cr.oracle_window(oracle, c, w, Y, Tw, yreal) for w in range(len(c.lens))])
    return _ORACLE[c.id]


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_oracle_accepts_the_case_and_its_forecasts_stand(oracle, c):
    Y, Tw, yreal, runs = oracle_runs(oracle, c)
    H = len(c.horizons)
    nd = c.sweeps[1] * (cr.N_SAMPLES if cr.is_sig(c) else 1)
    for w, o in enumerate(runs):
        assert o["status"] == 0, (c.id, w)
        assert o["fcast"].shape == (nd, 2 * H) and o["summary"].shape == (3 * c.K + c.K ** 2 + 2 * H,)
        unknown = np.isnan(o["fcast"])
        assert not unknown[:, 0::2].any() and np.array_equal(unknown[:, 1::2], np.broadcast_to(np.isnan(yreal[w]), (nd, H))), (c.id, w)
        if c.path != "tail":           # there pi_end is the smoothed row at end_pos, while the forecast starts from the last step
            d = cr.forecast_distance(o["fcast"], o["pi_end"], o["A"], o["mu"], c.horizons)
            assert d < ORACLE_FORECAST_BOUND, (c.id, w, d)
    if c.blend:
        other = tuple(7 if k in c.blend else h for k, h in enumerate(c.horizons))
        assert other != c.horizons
        for w, o in enumerate(runs):
            o2 = cr.oracle_window(oracle, c, w, Y, Tw, yreal, horizons=other)
            for k in ("fcast", "summary", "sample_summary", "mu", "pi_end"):
                assert np.array_equal(o[k], o2[k], equal_nan=True), (c.id, w, k)


def test_seed_high_word_changes_the_oracles_draws(oracle):
    c = cr.BY_ID["reg-K3-p1-H6"]
    assert c.seed == cr.SEED_HIGH_WORD
    Y, Tw, yreal, runs = oracle_runs(oracle, c)
    low = cr.oracle_window(oracle, c._replace(seed=cr.SEED_DEFAULT), 0, Y, Tw, yreal)
    assert not np.array_equal(low["mu"], runs[0]["mu"])
