"""hmcg_predictive_cdf[_device] on the GPU: the draw mean of the regime mixture's normal CDF (calc_cdfs.jl:39-41) and its
h-step-ahead form, from hand-made draws and from the sampler's own.

Reference (predictive_cases.reference): float64 numpy on the same arrays -- np.round(x, 5) with round5, omega by successive
vector-matrix products, Phi via math.erfc, np.mean.  Absolute tolerance (predictive_cases.tolerance, derived, not measured):
(nd + 64 + 2 K h_max) 2^-52.  NaN positions must match exactly.

Largest difference an MI355X run of this module showed: 2.442e-15 = 11 * 2^-52 (K = 2, nd = 1023, horizons (0, 1, 12), raw draws,
and K = 8, nd = 1025, horizons (12, 0)) against tolerances of 2.5e-13 and 2.8e-13 there; among the K = 4..7 cases 1.776e-15 =
8 * 2^-52 (K = 7, nd = 1025, horizons (0, 1, 12)) against 2.8e-13, and at each K's largest LDS tile (eight horizons, nd = 65) 2 to
3 * 2^-52 (6.7e-16 at K = 7) against 1.0e-13 to 1.5e-13.  As |diff| / tolerance the largest is 0.023 (K = 4, nd = 65, G = 65, raw draws: 6.7e-16 against
2.9e-14; K = 7, one draw: 3.3e-16 against 1.4e-14).  2.3e-15 between the device and the file route on the inflation data
(nd = 1500)."""
import datetime as dt

import numpy as np
import pytest

import predictive_cases as pc
import stat_device_entry as sde

pytestmark = pytest.mark.gpu


def _slab():
    from hmc_jl_amd import _lib
    return _lib.PRED_SLAB


def _device_cdf(mu, sig2, pi, A, grid, horizons, nd, round5=True):
    """The device entry over torch buffers (stat_device_entry.run): arrays with leading dimension mu.shape[2] >= nd."""
    return sde.run("predictive_cdf", dict(mu=mu, sig2=sig2, pi=pi, A=A, grid=grid, horizons=horizons, nd=nd, round5=round5))


def _cases():
    """A pruned product: K in {2, 3, 8} x nd around the tile (64) and the slab, with G in {1, 64, 65, 81}, W in {1, 3}, horizons
    (0,) with A = NULL or (0, 1, 12), nd_ld = nd or nd + 5 and round5 on / off dealt round-robin; then the corners the deal misses."""
    S = 1024                      # asserted equal to _lib.PRED_SLAB in the test
    Gs = (1, 64, 65, 81)
    out = []
    idx = 0
    for K in (2, 3, 8):
        for nd in (1, 63, 65, S - 1, S, S + 1, 2 * S + 17):
            G = Gs[idx % 4]
            W = 3 if nd <= 65 or G == 1 else 1
            out.append((K, nd, G, W, (0,) if idx % 2 == 0 else (0, 1, 12), 5 * ((idx // 2) % 2), (idx // 3) % 2 == 0))
            idx += 1
    out += [(3, 2 * S + 17, 81, 1, (0,), 5, True),            # the production form across slabs, padded
            (3, 2 * S + 17, 1, 3, (0, 1, 12), 0, True),        # several windows x several slabs
            (2, S + 1, 81, 3, (0, 1, 12), 5, False),
            (8, S + 1, 64, 1, (12, 0), 0, True),               # horizons in another order
            (3, 65, 81, 3, (0, 0, 1, 2, 3, 5, 8, 12), 5, True),    # HMCG_MAXH horizons: more than one block of items
            (8, 65, 65, 1, (0, 1, 2, 3, 5, 8, 12, 40), 0, False)]  # the largest LDS tile (73.7 KB)
    return out + _mid_k_cases()


NEW_KS = (4, 5, 6, 7)             # the K between the three above: other staging remainders, LDS offsets and unrollings
H8 = (0, 1, 2, 3, 5, 8, 12, 40)


def _mid_k_cases():
    """K = 4..7 at the smallest sizes that still meet every edge: one draw, one over the 64-draw tile, one over the slab, with
    G in {1, 65}, horizons (0,) with A = NULL or (0, 1, 12), nd_ld = nd or nd + 5 and round5 on / off dealt so that every K
    meets each (tests/test_stat_coverage.py checks the deal); then per K its largest LDS tile: eight horizons with A, a partial
    grid block, a partial draw tile (K = 7: 60 928 B, past the 48 KB that need the attribute call of HMCG_LAUNCH_LDS)."""
    out = []
    idx = 0
    for K in NEW_KS:
        for nd in (1, 65, 1025):
            out.append((K, nd, (1, 65)[idx % 2], 3 if nd <= 65 else 1, (0,) if (idx // 2) % 2 == 0 else (0, 1, 12),
                        5 * ((idx + idx // 3) % 2), ((idx + 1) // 2) % 2 == 0))
            idx += 1
    return out + [(K, 65, 65, 1, H8, 5 * (K % 2), K % 2 == 0) for K in NEW_KS]


@pytest.mark.parametrize("K,nd,G,W,horizons,pad,round5", _cases())
def test_device_entry_against_reference(K, nd, G, W, horizons, pad, round5):
    assert _slab() == 1024
    with_A = max(horizons) > 0
    mu, sig2, pi, A = pc.make_draws(1000 * K + nd + G, W, K, nd, pad, with_A)
    grid = pc.make_grid(G)
    exp = pc.reference(mu, sig2, pi, A, grid, horizons, round5, nd)
    assert np.isfinite(exp).all()
    got = _device_cdf(mu, sig2, pi, A, grid, horizons, nd, round5)
    assert got.shape == exp.shape and np.array_equal(np.isnan(got), np.isnan(exp))
    err = float(np.abs(got - exp).max())
    print("K=%d nd=%d G=%d W=%d h=%s pad=%d round5=%s: max |diff| = %.3e (%.1f 2^-52), tol %.3e"
          % (K, nd, G, W, horizons, pad, round5, err, err * 2.0 ** 52, pc.tolerance(nd, K, max(horizons))))
    assert err <= pc.tolerance(nd, K, max(horizons))


def test_ieee_edge_cases():
    """No special-casing: a rounded variance of 0 gives Phi = 0 or 1 beside the mean and NaN on it; a NaN term under a zero
    weight still makes its cell NaN; |z| > 40 gives exactly 0 and exactly 1; the grid needs no order."""
    K, nd, W = 2, 70, 2
    mu, sig2, pi, _ = pc.make_draws(5, W, K, nd, 0, False)
    grid = np.array([1.25, 1.5, 1.75, 6.0])
    # window 0: draw 3's state 0 has variance 4e-6 -> 0.0 once rounded, mean 1.5 = grid[1]
    mu[0, 0, 3], sig2[0, 0, 3] = 1.5, 4e-6
    # window 1: draw 9's state 1 has a NaN mean under a weight of exactly 0
    mu[1, 1, 9], pi[1, 0, 9], pi[1, 1, 9] = np.nan, 1.0, 0.0
    exp = pc.reference(mu, sig2, pi, None, grid, (0,), True)
    got = _device_cdf(mu, sig2, pi, None, grid, (0,), nd, True)
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    assert np.isnan(got[0, 0, 1]) and np.isfinite(got[0, 0, [0, 2, 3]]).all() and np.isnan(got[1]).all()
    ok = ~np.isnan(exp)
    assert np.abs(got[ok] - exp[ok]).max() <= pc.tolerance(nd, K, 0)
    # without the rounding the variance is 4e-6, not 0: every cell of window 0 is finite
    raw = _device_cdf(mu, sig2, pi, None, grid, (0,), nd, False)
    assert np.isfinite(raw[0]).all() and np.abs(raw[0] - pc.reference(mu, sig2, pi, None, grid, (0,), False)[0]).max() <= pc.tolerance(nd, K, 0)
    # |z| = 50 on both sides, weights 0.5 + 0.5: exactly 0 and exactly 1
    mu2, sig22 = np.zeros((1, 2, 33)), np.full((1, 2, 33), 0.01)
    pi2 = np.full((1, 2, 33), 0.5)
    far = _device_cdf(mu2, sig22, pi2, None, np.array([-5.0, 5.0]), (0,), 33, True)
    assert far[0, 0, 0] == 0.0 and far[0, 0, 1] == 1.0
    # an unsorted grid: every point is computed on its own
    mu3, sig23, pi3, _ = pc.make_draws(6, 1, 3, 200, 0, False)
    g = pc.make_grid(65)
    perm = np.random.default_rng(2).permutation(65)
    a = _device_cdf(mu3, sig23, pi3, None, g, (0,), 200)
    b = _device_cdf(mu3, sig23, pi3, None, g[perm], (0,), 200)
    assert np.array_equal(b, a[:, :, perm])


def test_host_entry_equals_device_entry_bit_for_bit(monkeypatch):
    """One slab cut for both entries and for every chunking of the host entry's upload: the same bits."""
    from hmc_jl_amd import _lib
    S = _lib.PRED_SLAB
    K, W, nd = 3, 2, 3 * S + 17
    horizons = (0, 1, 12)
    mu, sig2, pi, A = pc.make_draws(77, W, K, nd, 0, True)
    grid = pc.make_grid(81)
    dev = _device_cdf(mu, sig2, pi, A, grid, horizons, nd)
    tm = _lib.Timing()
    one = _lib.predictive_cdf_host(mu, sig2, pi, A, grid, horizons, timing=tm)
    assert tm.launches == 2 and tm.kernel_ms > 0.0 and tm.call_ms >= tm.kernel_ms
    monkeypatch.setenv("HMCG_CHUNK_DRAWS", str(S + 476))         # no slab multiple: rounded up to 2 slabs -> 2 chunks
    two = _lib.predictive_cdf_host(mu, sig2, pi, A, grid, horizons, timing=tm)
    assert tm.launches == 3
    monkeypatch.setenv("HMCG_CHUNK_DRAWS", "1")                  # one slab per chunk: 4 chunks through a ring of 3 buffers
    four = _lib.predictive_cdf_host(mu, sig2, pi, A, grid, horizons, timing=tm)
    assert tm.launches == 5
    monkeypatch.delenv("HMCG_CHUNK_DRAWS")
    again = _lib.predictive_cdf_host(mu, sig2, pi, A, grid, horizons)
    for o in (one, two, four, again):
        assert np.array_equal(o, dev)
    assert np.array_equal(_device_cdf(mu, sig2, pi, A, grid, horizons, nd), dev)
    assert np.abs(dev - pc.reference(mu, sig2, pi, A, grid, horizons, True)).max() <= pc.tolerance(nd, K, 12)
    # horizon 0 alone: A is neither needed nor uploaded
    h0 = _lib.predictive_cdf_host(mu, sig2, pi, None, grid, (0,))
    assert np.array_equal(h0[:, 0], dev[:, 0])


@pytest.mark.parametrize("K,T,nrun", [(3, 200, 700), (8, 700, 200), (5, 300, 200)])
def test_device_panel_predictive_cdf(K, T, nrun):
    """DevicePanel.predictive_cdf on the draws `run` left in HBM (K = 8 / T = 700 runs the LDS-resident kernel, whose scratch
    shares the device context with the slab sums); the draws are unchanged afterwards."""
    from hmc_jl_amd import _lib, synth
    from hmc_jl_amd.device import DevicePanel
    W = 3
    Y, Tw, fut = synth.generate_panel(W, T, K)
    p = DevicePanel(Y, Tw, K, nrun, (12,), fut[:, 11:12])
    p.run(burnin=20, timed=False)
    grid = np.arange(-5, 15.25, .25)
    horizons = (0, 12)
    cdf = p.predictive_cdf(grid, horizons)                   # enqueued behind the run on the library stream
    p.sync()
    before = {n: getattr(p, n).cpu().numpy() for n in _lib.DRAW_KEYS}
    assert (p.status.cpu().numpy() == 0).all()
    timed = p.predictive_cdf(grid, horizons, timed=True)
    assert p.last_timing.kernel_ms > 0.0
    got = cdf.cpu().numpy()
    assert got.shape == (W, 2, 81) and np.array_equal(got, timed.cpu().numpy())
    exp = pc.reference(before["mu"], before["sig2"], before["pi_end"], before["A"], grid, horizons, True)
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    assert np.abs(got - exp).max() <= pc.tolerance(nrun, K, 12)
    for n in _lib.DRAW_KEYS:
        assert np.array_equal(getattr(p, n).cpu().numpy(), before[n])
    with pytest.raises(_lib.HmcgError, match="keep_draws"):
        DevicePanel(Y, Tw, K, nrun, (12,), fut[:, 11:12], keep_draws=False).predictive_cdf(grid)


def test_estimatewindows_cdf_equals_the_file_route(inflation, tmp_path):
    """code/run_hmm.jl's windows for two end dates: BatchResult.cdf from the device against calc_cdfs.jl's route over the
    per-draw files saveresults writes; and the same bits when the draws are not kept."""
    from hmc_jl_amd import hmc
    y, dates = inflation
    dd = [dt.date.fromisoformat(d) for d in dates]
    ends = [200, 201]
    ys = np.arange(-5, 15.25, .25)
    kw = dict(horizons=[12], D=3, burnin=300, Nrun=1500, series="official", cdf_grid=ys, cdf_horizons=(0, 12))
    res = hmc.estimatewindows(y, dd, ends, keep_draws=True, **kw)
    assert (res.status == 0).all() and res.cdf.shape == (2, 2, 81) and np.array_equal(res.cdf_grid, ys)
    for w in range(2):
        hmc.saveresults(res.samples(w), res.opts[w], str(tmp_path))
    want = [dd[e - 1] for e in ends]
    d_f, ys_f, bar_f, fin_f = hmc.calccdfs(str(tmp_path), want, ys, (0, 12))
    d_d, ys_d, bar_d, fin_d = hmc.calccdfs(str(tmp_path), want, ys, (0, 12), result=res)
    assert d_f == d_d == [str(d) for d in want] and np.array_equal(bar_d, res.cdf)
    assert np.isfinite(bar_f).all() and np.isfinite(bar_d).all()
    err = float(np.abs(bar_f - bar_d).max())
    print("device vs file route: max |diff| = %.3e (%.1f 2^-52)" % (err, err * 2.0 ** 52))
    assert err <= pc.tolerance(1500, 3, 12)
    assert (np.diff(bar_d, axis=2) >= -1e-15).all()           # a CDF on an ascending grid
    lean = hmc.estimatewindows(y, dd, ends, keep_draws=False, **kw)
    assert np.array_equal(lean.cdf, res.cdf)
    with pytest.raises(ValueError):
        lean.samples(0)
