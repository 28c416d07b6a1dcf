"""The shared comparison (tests/oracle_parity.py) and the shared tables (tests/kernel_tables.py) are single points of failure of
the GPU suite: this pins, without a GPU and without the oracle, that the comparison is strict.  A synthetic result g in the C-ABI
layouts and its oracle counterpart o per window (W = 2, K = 3, T = (5, 7), nrun = 4, H = 2, one forecast-error column unknown
in both) pass; one cell of any compared field moved by 2 TOL (1 + |x|) fails with the field's name in the message, moved by
TOL (1 + |x|) / 2 it passes; a state flipped inside T fails, beyond T it does not; NaN on one side only fails."""
import numpy as np
import pytest

import kernel_tables as kt
import oracle_parity as op
from oracle_parity import TOL, assert_same, assert_window_matches_oracle

W, K, TW, NRUN, H, LD, NSAVE, NSAVE_LD = 2, 3, (5, 7), 4, 2, 7, 2, 3
NS = 3 * K + K * K + 2 * H
PLAIN = ("mu", "sig2", "A", "pi_end", "pif_final", "pi_smooth_mean", "pi_filter_mean", "pi_smooth_draws", "sigvals")
WITH_NAN = ("fcast", "summary", "sample_summary")
FIELDS = dict(fields=PLAIN, nan_fields=WITH_NAN, nsave=NSAVE)


def simplex(rng, *shape):
    p = rng.uniform(0.1, 1.0, shape)
    return p / p.sum(axis=-1, keepdims=True)


def make_pair(unknown=True):
    """(g, [o of window 0, o of window 1]): the same numbers in the library's layouts and in the oracle's."""
    rng = np.random.default_rng(7)
    outs = []
    for T in TW:
        o = dict(mu=rng.normal(0, 3, (NRUN, K)), sig2=rng.uniform(0.5, 2, (NRUN, K)), A=simplex(rng, NRUN, K, K), pi_end=simplex(rng, NRUN, K),
                 fcast=rng.normal(0, 2, (NRUN, 2 * H)), summary=rng.normal(0, 2, NS), pif_final=simplex(rng, T, K),
                 x_final=rng.integers(0, K, T).astype(np.int32), status=0, pi_smooth=simplex(rng, NRUN, T, K), pi_filter_mean=simplex(rng, T, K),
                 sigvals=rng.normal(0, 1, (1, NSAVE)), sample_summary=rng.normal(0, 2, (1, NS)))
        if unknown:                                  # the error column of horizon slot 0, and its rows of the summaries
            o["fcast"][:, 1] = o["summary"][NS - 2 * H + 1] = o["sample_summary"][:, NS - 2 * H + 1] = np.nan
        outs.append(o)

    def padded(rows, fill):
        out = np.full((W, LD) + rows[0].shape[1:], fill, dtype=rows[0].dtype)
        for w, r in enumerate(rows):
            out[w, :len(r)] = r
        return out

    g = {k: np.stack([np.ascontiguousarray(o[k].T) for o in outs]) for k in ("mu", "sig2", "pi_end", "fcast")}
    g["A"] = np.stack([np.transpose(o["A"], (2, 1, 0)) for o in outs])
    g["summary"], g["sample_summary"] = np.stack([o["summary"] for o in outs]), np.stack([o["sample_summary"] for o in outs])
    g["status"] = np.zeros(W, np.int32)
    g["x_final"] = padded([o["x_final"] for o in outs], 0)
    for k in ("pif_final", "pi_filter_mean"):
        g[k] = padded([o[k] for o in outs], 0.0)
    g["pi_smooth_mean"] = padded([o["pi_smooth"].mean(axis=0) for o in outs], 0.0)
    g["pi_smooth_draws"] = np.zeros((W, K, LD, NRUN))
    g["sigvals"] = np.full((W, 1, NSAVE_LD), -7.25)                       # beyond the saved positions: not the oracle's business
    for w, o in enumerate(outs):
        g["pi_smooth_draws"][w, :, :TW[w], :] = np.transpose(o["pi_smooth"], (2, 1, 0))
        g["sigvals"][w, :, :NSAVE] = o["sigvals"]
    return g, outs


def moved(g, k, w, factor):
    """A copy of g with one cell of field k of window w (inside the window's T steps and saved positions, not an unknown one)
    moved by factor * TOL * (1 + |x|)."""
    g = dict(g, **{k: g[k].copy()})
    view = op.window_view(g, w, TW[w], k, NSAVE)                          # a view into the copy
    cell = tuple(int(i) for i in np.argwhere(~np.isnan(view))[-1])
    view[cell] += factor * TOL * (1.0 + abs(view[cell]))
    return g


def test_unperturbed_pair_passes_with_every_field():
    g, outs = make_pair()
    for w, T in enumerate(TW):
        assert_window_matches_oracle(g, w, T, outs[w], **FIELDS)
        assert_window_matches_oracle(g, w, T, outs[w], fields=PLAIN[:5], known_fields=WITH_NAN)


@pytest.mark.parametrize("k", PLAIN + WITH_NAN)
@pytest.mark.parametrize("w", range(W))
def test_one_moved_cell_of_each_field(k, w):
    g, outs = make_pair()
    with pytest.raises(AssertionError, match="window %d: %s differs" % (w, k)):
        assert_window_matches_oracle(moved(g, k, w, 2.0), w, TW[w], outs[w], **FIELDS)
    assert_window_matches_oracle(moved(g, k, w, 0.5), w, TW[w], outs[w], **FIELDS)
    assert_window_matches_oracle(g, 1 - w, TW[1 - w], outs[1 - w], **FIELDS)      # (the other window is not touched)
    if k in WITH_NAN:                                                           # the cells the oracle knows, whatever g holds in the others
        with pytest.raises(AssertionError, match="%s differs" % k):
            assert_window_matches_oracle(moved(g, k, w, 2.0), w, TW[w], outs[w], fields=(), known_fields=(k,))


def test_states_and_status():
    g, outs = make_pair()
    inside, beyond = dict(g, x_final=g["x_final"].copy()), dict(g, x_final=g["x_final"].copy())
    inside["x_final"][0, TW[0] - 1] = (inside["x_final"][0, TW[0] - 1] + 1) % K
    beyond["x_final"][0, TW[0]] += 1
    with pytest.raises(AssertionError, match="x_final"):
        assert_window_matches_oracle(inside, 0, TW[0], outs[0], **FIELDS)
    assert_window_matches_oracle(beyond, 0, TW[0], outs[0], **FIELDS)
    assert_window_matches_oracle(inside, 0, TW[0], outs[0], states=False, **FIELDS)
    flagged = dict(g, status=np.array([0, 2], np.int32))
    with pytest.raises(AssertionError, match="status"):
        assert_window_matches_oracle(flagged, 1, TW[1], outs[1], **FIELDS)
    with pytest.raises(AssertionError, match="status"):                         # equal, but not 0
        assert_window_matches_oracle(flagged, 1, TW[1], dict(outs[1], status=2), **FIELDS)
    assert_window_matches_oracle(flagged, 1, TW[1], dict(outs[1], status=2), status0=False, **FIELDS)


def test_nan_on_one_side_only():
    g, outs = make_pair()
    assert op.close_nan(g["fcast"][0].T, outs[0]["fcast"]) < TOL
    lost = dict(g, fcast=g["fcast"].copy())
    lost["fcast"][0, 0, 2] = np.nan                                             # NaN in the result alone
    with pytest.raises(AssertionError, match="fcast differs"):
        assert_window_matches_oracle(lost, 0, TW[0], outs[0], **FIELDS)
    known = dict(g, fcast=g["fcast"].copy())
    known["fcast"][0, 1, 2] = 0.0                                               # NaN in the oracle alone
    with pytest.raises(AssertionError, match="fcast differs"):
        assert_window_matches_oracle(known, 0, TW[0], outs[0], **FIELDS)
    assert op.close_nan(lost["fcast"][0].T, outs[0]["fcast"]) == op.close_nan(known["fcast"][0].T, outs[0]["fcast"]) == float("inf")
    with pytest.raises(AssertionError, match="fcast differs"):                  # close() itself never passes a NaN
        assert_window_matches_oracle(g, 0, TW[0], outs[0], fields=("fcast",))


def test_assert_same():
    g, _ = make_pair()
    h = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in g.items()}
    assert_same(g, h)
    assert_same(g, h, ("mu", "fcast", "x_final"))
    with pytest.raises(AssertionError, match="fcast"):                          # NaN equals NaN only when asked to
        assert_same(g, h, ("mu", "fcast"), equal_nan=False)
    assert_same(g, h, ("mu", "x_final"), equal_nan=False)
    h["sig2"][1, 2, 3] = np.nextafter(h["sig2"][1, 2, 3], np.inf)
    assert_same(g, h, ("mu", "fcast", "x_final"))
    with pytest.raises(AssertionError, match="sig2"):
        assert_same(g, h, what="one ulp")
    with pytest.raises(AssertionError, match="sig2"):
        assert_same(g, h, ("mu", "sig2"))
    with pytest.raises(AssertionError, match="corr"):                           # every array: both hold the same ones
        assert_same(g, dict(g, corr=np.zeros(3)))


class StubOracle:
    """estimate_window / estimate_signals that hand back the synthetic o of the window whose length they are given."""

    def __init__(self, outs):
        self.by_length = {len(o["x_final"]): o for o in outs}

    def estimate_window(self, Y, *a, **kw):
        return dict(self.by_length[len(Y)])

    estimate_signals = estimate_window


def test_checkers_pass_on_the_pair():
    g, outs = make_pair()
    Y, Tw = np.zeros((W, LD)), np.array(TW, dtype=np.int32)
    yreal = np.array([[np.nan, 1.0]] * W)
    ends = np.stack([Tw - NSAVE, Tw], axis=1)
    oracle, run = StubOracle(outs), lambda *a, **kw: g
    assert op.check_against_oracle(oracle, Y, Tw, K, 1, NRUN, (1, 12), yreal, run=run) is g
    assert op.check_signals_against_oracle(oracle, Y, Tw, K, 1, NRUN, 1, ends, ends, 0.6, 2.0, 2.0, np.ones(W), yreal, run=run, horizons=(1, 12)) is g
    assert op.check_tail_signals_against_oracle(oracle, Y, Tw, K, 1, NRUN, 1, ends, ends, np.ones(W), Tw - 2, (0, 12), yreal, NSAVE,
                                                want_sample_summary=True, run=run) is g
    last = {k: (v[1:] if isinstance(v, np.ndarray) else v) for k, v in g.items()}       # the full-length window alone
    op.check_teacher_forced_against_oracle(oracle, Y[1:], Tw[1:], K, np.zeros((1, LD), np.int32), run=lambda *a, **kw: last)
    # a checker fails with the comparison: one moved cell
    with pytest.raises(AssertionError, match="window 1: pi_end differs"):
        op.check_against_oracle(oracle, Y, Tw, K, 1, NRUN, (1, 12), yreal, run=lambda *a, **kw: moved(g, "pi_end", 1, 2.0))
    # check_smoothing_against_oracle compares fcast and summary through close(): every realised value known
    g, outs = make_pair(unknown=False)
    oracle, run = StubOracle(outs), lambda *a, **kw: g
    op.check_smoothing_against_oracle(oracle, Y, Tw, K, 1, NRUN, yreal, run=run)
    op.check_smoothing_against_oracle(oracle, Y, Tw, K, 1, NRUN, yreal, sig=ends, ssig=np.ones(W), run=run)
    with pytest.raises(AssertionError, match="window 0: pi_smooth_draws differs"):
        op.check_smoothing_against_oracle(oracle, Y, Tw, K, 1, NRUN, yreal, run=lambda *a, **kw: moved(g, "pi_smooth_draws", 0, 2.0))


# ---- tests/kernel_tables.py ----
def test_steps_per_thread_agrees_with_the_parsed_classes():
    paths = sorted({(K, sig, sm) for (K, L, nt, sig, sm, _, _) in kt.REG_ROWS if nt == kt.NT})
    assert len(paths) >= 12
    for (K, sig, sm) in paths:
        classes = kt.register_classes(K, sig, sm)
        assert classes == sorted(set(classes)) and classes
        for L, above in zip(classes, classes[1:] + [None]):
            assert kt.steps_per_thread(K, kt.NT * L, sig, sm) == L
            if above is None:                        # beyond the ladder: the LDS-resident kernel's
                assert kt.NT * L == kt.ladder_ceiling(K, sig, sm)
                with pytest.raises(ValueError):
                    kt.steps_per_thread(K, kt.NT * L + 1, sig, sm)
            else:
                assert kt.steps_per_thread(K, kt.NT * L + 1, sig, sm) == above
        assert kt.steps_per_thread(K, 2, sig, sm) == classes[0]


def test_flavour_table_is_the_expansion_of_a_three_flavour_row():
    """HMCG_V3 alone expands to several (NH, OCC) of one (K, L, NT, sig, smooth): the three of FLAVOUR_WAVES."""
    by_row = {}
    for r in kt.REG_ROWS:
        by_row.setdefault(r[:5], []).append(r[5:])
    three = {row: fl for row, fl in by_row.items() if len(fl) > 1}
    assert three and all(sorted(fl) == sorted(kt.FLAVOUR_WAVES.values()) for fl in three.values())
    assert sorted(kt.VARIANT_ROWS) == sorted((K, L, {v: k for k, v in kt.PATH.items()}[sig, sm]) for (K, L, nt, sig, sm) in three)
    assert sorted(kt.VARIANT_CASES) == sorted((K, L, p, fl) for (K, L, p) in kt.VARIANT_ROWS for fl in kt.FLAVOUR_WAVES)


def test_parsed_ladders_give_the_case_lists_their_modules_were_written_for():
    """test_gpu_wave_prefix's cases are the base-path classes of K = 2, 3, 4: the parsed ones equal the list its ids carry.
    test_gpu_param_overlap's lengths were chosen on the ladder 1, 2, 4, 8: the parsed ladder, which also holds 3, 6 and 12, gives
    each of them the same class."""
    assert {K: tuple(kt.register_classes(K, False, False)) for K in (2, 3, 4)} == {2: (1, 2, 3, 4, 8), 3: (1, 2, 3, 4, 6, 8, 12, 16), 4: (1, 2, 3, 4, 8)}
    for K in (2, 3, 4):
        for T in (2, 37, 63, 64, 65, 511, 1023, 2047):
            assert kt.steps_per_thread(K, T) == (1 if T <= 256 else 2 if T <= 512 else 4 if T <= 1024 else 8), (K, T)
    assert sorted(kt.OWN_THREAD_COUNT) == [(3, 2, 512), (3, 8, 128)]
