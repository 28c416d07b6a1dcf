"""hmcg_bias_moments[_device] on the GPU: mean and covariance over the draws of [pi_end A^h | mu] and the two numbers
bias_calcs.jl:40-53 reduces them to, from hand-made draws and from the sampler's own.

Reference (bias_cases.reference): np.longdouble on the same arrays, np.round(x, 5) with round5, upstream's index swap in uncbias.
Per-cell absolute tolerance (bias_cases.tolerance, derived, not measured): cov (3 n + 7) 2^-52 R_a R_b + 4 (R_a e_b + R_b e_a),
R = max |v - v_0| per column; mean, uncbias and totalbias follow from it.  NaN positions must match exactly.

Largest differences an MI355X run of this module showed, as |diff| / its bound: cov 0.055 (K = 8, nd = 2, h = 12: 6.7e-16
against 1.2e-14), among K = 4..7 0.042 (K = 7, nd = 2, h = 12: 6.2e-16 against 1.5e-14), the largest absolute one 1.06e-14 against
1.4e-10 (K = 8, nd = 2065, raw draws); uncbias 0.019 (2.4e-15 against 1.2e-13, K = 6, nd = 2, h = 0); totalbias 0.23 (1.1e-16
against 4.9e-16, K = 4, nd = 2: one rounding); mean 0.79 in the offset case (8.8e-13 against 1.1e-12: one rounding of a value near
1e4), in the case table 0.63 (K = 7, nd = 2, h = 12: 4.4e-16, one rounding, against 9.8e-16).  Predictive CDF against mean[0:K] on a one-hot mixture: 3.3e-16
against 4.4e-13.  Device against file route on the inflation data (nd = 1500): cov 1.3e-17 and 2.9e-17 from the reference."""
import datetime as dt

import numpy as np
import pytest

import bias_cases as bc
import stat_device_entry as sde

pytestmark = pytest.mark.gpu


def _device_bias(mu, pi, A, fc, horizon, nd, round5=True, timed=True):
    """The device entry over torch buffers (stat_device_entry.run): arrays with leading dimension mu.shape[2] >= nd.  Returns
    the unpacked output and the raw [W][stride] block; the sentinel rows before and after it are checked there."""
    return sde.run("bias_moments", dict(mu=mu, pi=pi, A=A, fc=fc, horizon=horizon, nd=nd, round5=round5), timed)


def _cases():
    """A pruned product: K in {2, 3, 8} x every nd of the issue (around the 64-lane tile and the slab), with W in {1, 3}, horizon
    in {0 (A = NULL), 1, 12}, nd_ld = nd or nd + 5, round5 on / off and fcast NULL / H = 1 / H = 2 dealt round-robin, then the
    corners the deal misses."""
    S = 1024                      # asserted equal to _lib.PRED_SLAB in the test
    out = []
    idx = 0
    for K in (2, 3, 8):
        for nd in (1, 2, 63, 65, S - 1, S, S + 1, 2 * S + 17):
            out.append((K, nd, 3 if nd <= 65 else 1, (0, 1, 12)[idx % 3], 5 * ((idx // 2) % 2), (idx // 3) % 2 == 0, (1, 0, 2)[(idx // 2) % 3]))
            idx += 1
    out += [(3, 2 * S + 17, 3, 12, 5, True, 1),            # the production form: several windows x several slabs, padded
            (8, 2 * S + 17, 3, 12, 0, False, 2),
            (2, S + 1, 3, 0, 5, True, 0),
            (3, 1, 1, 12, 0, True, 1),                     # nd = 1 at the reference's own horizon
            (8, 2, 1, 12, 5, True, 2),
            (3, S, 1, 12, 0, False, 0)]
    return out + _mid_k_cases()


NEW_KS = (4, 5, 6, 7)             # the K between the three above: items mod 4 = 1, 2, 3, 0; K = 6, 7 on the non-unrolled path


def _mid_k_cases():
    """K = 4..7 at the smallest sizes that still meet every edge: two draws, one over a lane's first draw (a lane takes draws l,
    l + 64, l + 128, l + 192 of the 256-draw tile), one over the tile, one over the slab, one over two slabs and a tile; horizon
    0 (A = NULL) or 12, with or without the forecast-error column, nd_ld = nd or nd + 5 and round5 on / off dealt so that every
    K meets each (tests/test_stat_coverage.py checks the deal)."""
    out = []
    idx = 0
    for K in NEW_KS:
        for nd in (2, 65, 257, 1025, 2065):
            out.append((K, nd, 3 if nd <= 65 else 1, (0, 12)[idx % 2], 5 * ((idx // 2) % 2), (idx // 3) % 2 == 0, (1, 0)[((idx + 1) // 2) % 2]))
            idx += 1
    return out


@pytest.mark.parametrize("K,nd,W,horizon,pad,round5,H", _cases())
def test_device_entry_against_reference(K, nd, W, horizon, pad, round5, H):
    from hmc_jl_amd import _lib
    assert _lib.PRED_SLAB == 1024
    mu, pi, A, fc = bc.make_draws(1000 * K + nd + 31 * horizon, W, K, nd, pad, horizon > 0, H)
    ref = bc.reference(mu, pi, A, fc, horizon, round5, nd)
    got, raw = _device_bias(mu, pi, A, fc, horizon, nd, round5)
    if nd == 1:
        assert np.isnan(got["cov"]).all() and np.isnan(got["uncerbias"]).all() and np.isfinite(got["mean"]).all()
    else:
        assert np.isfinite(got["cov"]).all() and np.isfinite(got["uncerbias"]).all()
    assert np.isnan(got["totalbias"]).all() if H == 0 else np.isfinite(got["totalbias"]).all()
    bc.check(got, ref, bc.tolerance(ref, nd, K, horizon), "K=%d nd=%d W=%d h=%d pad=%d r5=%s H=%d" % (K, nd, W, horizon, pad, round5, H))
    c = got["cov"]
    assert np.array_equal(c.view(np.uint64), np.transpose(c, (0, 2, 1)).copy().view(np.uint64)), "cov is not bit-symmetric"


def test_identical_draws_give_exact_zeros():
    """Every draw equal to draw 0 (the pivot): v - p is exactly 0, so cov and uncbias are exactly 0.0."""
    K, nd, W = 3, 1100, 2
    mu, pi, A, fc = bc.make_draws(8, W, K, 1, 0, True, 1)
    rep = lambda a: np.repeat(a, nd, axis=-1)
    got, _ = _device_bias(rep(mu), rep(pi), rep(A), rep(fc), 12, nd)
    assert (got["cov"] == 0.0).all() and (got["uncerbias"] == 0.0).all()
    ref = bc.reference(rep(mu), rep(pi), rep(A), rep(fc), 12, True)
    bc.check(got, ref, bc.tolerance(ref, nd, K, 12), "identical")
    assert np.array_equal(got["totalbias"], np.round(fc[:, 1, 0], 5))


def test_large_offset_costs_no_digits():
    """Means at 1e4 plus a spread of 1e-2: the derived tolerance scales with the spread about draw 0 (R ~ 1e-2), not with the
    offset -- a sum of raw squares would lose 12 digits here."""
    K, nd, W = 3, 1500, 2
    mu, pi, A, fc = bc.make_draws(9, W, K, nd, 0, True, 1)
    mu = 1e4 + 1e-2 * (mu - 2.0) / 3.0
    ref = bc.reference(mu, pi, A, fc, 12, False)
    tol = bc.tolerance(ref, nd, K, 12)
    assert tol["cov"][:, K:, K:].max() < 1e-13 and ref["cov"][:, K:, K:].max() > 1e-6
    got, _ = _device_bias(mu, pi, A, fc, 12, nd, False)
    bc.check(got, ref, tol, "offset 1e4")


def test_one_nan_mean_poisons_its_row_and_column_only():
    K, nd, W = 3, 1030, 1
    mu, pi, A, fc = bc.make_draws(10, W, K, nd, 0, True, 1)
    mu[0, 1, 1027] = np.nan
    got, _ = _device_bias(mu, pi, A, fc, 12, nd)
    bad = K + 1                                           # column of mu_2 in futstate | means
    nanc = np.isnan(got["cov"][0])
    exp = np.zeros((2 * K, 2 * K), dtype=bool)
    exp[bad, :] = exp[:, bad] = True
    assert np.array_equal(nanc, exp)
    assert np.array_equal(np.isnan(got["mean"][0]), np.arange(2 * K) == bad)
    assert np.isnan(got["uncerbias"][0]) and np.isfinite(got["totalbias"][0])
    ref = bc.reference(mu, pi, A, fc, 12, True)
    bc.check(got, ref, bc.tolerance(ref, nd, K, 12), "one NaN")


def test_host_entry_equals_device_entry_bit_for_bit(monkeypatch):
    """One slab cut and one pivot for both entries and for every chunking of the host entry's upload: the same bits."""
    from hmc_jl_amd import _lib
    S = _lib.PRED_SLAB
    K, W, nd = 3, 2, 3 * S + 17
    mu, pi, A, fc = bc.make_draws(77, W, K, nd, 0, True, 2)
    _, dev = _device_bias(mu, pi, A, fc, 12, nd)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    tm = _lib.Timing()
    one = _lib.bias_moments_host(mu, pi, A, fc, 12, timing=tm)
    assert tm.launches == 2 and tm.kernel_ms > 0.0 and tm.call_ms >= tm.kernel_ms
    monkeypatch.setenv("HMCG_CHUNK_DRAWS", str(S + 476))         # no slab multiple: rounded up to 2 slabs -> 2 chunks
    two = _lib.bias_moments_host(mu, pi, A, fc, 12, timing=tm)
    assert tm.launches == 3
    monkeypatch.setenv("HMCG_CHUNK_DRAWS", "1")                  # one slab per chunk: 4 chunks through a ring of 3 buffers
    four = _lib.bias_moments_host(mu, pi, A, fc, 12, timing=tm)
    assert tm.launches == 5
    monkeypatch.delenv("HMCG_CHUNK_DRAWS")
    again = _lib.bias_moments_host(mu, pi, A, fc, 12)
    for o in (one, two, four, again):
        assert np.array_equal(bits(o), bits(dev))
    assert np.array_equal(bits(_device_bias(mu, pi, A, fc, 12, nd, timed=False)[1]), bits(dev))
    ref = bc.reference(mu, pi, A, fc, 12, True)
    bc.check(_lib.unpack_bias(four, K), ref, bc.tolerance(ref, nd, K, 12), "host, 4 chunks")
    # horizon 0 without A and without fcast, chunked: neither is needed nor uploaded
    monkeypatch.setenv("HMCG_CHUNK_DRAWS", "1")
    h0 = _lib.bias_moments_host(mu, pi, None, None, 0)
    monkeypatch.delenv("HMCG_CHUNK_DRAWS")
    _, d0 = _device_bias(mu, pi, None, None, 0, nd)
    assert np.array_equal(bits(h0), bits(d0)) and np.isnan(h0[:, 1]).all()


def test_same_omega_as_the_predictive_feature():
    """mean[0:K] is the draw mean of omega = pi_end A^h, and so is a predictive CDF under a one-hot mixture: state k at 0, the
    others at 100, unit variances, grid point 50 -- Phi is exactly 1 for state k and exactly 0 for the others, so the CDF is the
    draw mean of omega_k as hmcg_predictive_cdf builds it.  Both features build omega by the same expression; the two means then
    differ by their summations alone: the predictive sum of nd values in [0, 1] and its division, (nd + 1) 2^-53; the pivoted sum
    (nd + 1) 2^-53 R with R <= 1, and 2^-53 for p + S1 / n.  No share for the h-step recurrence."""
    from hmc_jl_amd import _lib
    K, nd, W, h = 3, 2000, 2, 12
    mu, pi, A, _ = bc.make_draws(12, W, K, nd, 0, True, 0)
    got, _ = _device_bias(mu, pi, A, None, h, nd)
    bound = (2 * nd + 3) * 2.0 ** -53
    for k in range(K):
        hot = np.full_like(mu, 100.0)
        hot[:, k, :] = 0.0
        cdf = _lib.predictive_cdf_host(hot, np.ones_like(mu), pi, A, np.array([50.0]), (h,))
        diff = np.abs(cdf[:, 0, 0] - got["mean"][:, k])
        print("omega_%d mean, predictive vs bias: max |diff| = %.3e, bound %.3e" % (k, diff.max(), bound))
        assert (diff <= bound).all() and (cdf[:, 0, 0] > 0.01).all()


@pytest.mark.parametrize("K,T,nrun", [(3, 200, 700), (8, 700, 200), (5, 300, 200)])
def test_device_panel_bias_moments(K, T, nrun):
    """DevicePanel.bias_moments on the draws `run` left in HBM (K = 8 / T = 700 runs the LDS-resident kernel, whose scratch
    shares the device context with the slab sums); the draws are unchanged afterwards."""
    from hmc_jl_amd import _lib, synth
    from hmc_jl_amd.device import DevicePanel
    W = 3
    Y, Tw, fut = synth.generate_panel(W, T, K)
    p = DevicePanel(Y, Tw, K, nrun, (12,), fut[:, 11:12])
    p.run(burnin=20, timed=False)
    out = p.bias_moments(12)                                 # enqueued behind the run on the library stream
    p.sync()
    before = {n: getattr(p, n).cpu().numpy() for n in _lib.DRAW_KEYS}
    assert (p.status.cpu().numpy() == 0).all()
    timed = p.bias_moments(12, timed=True)
    assert p.last_timing.kernel_ms > 0.0 and p.last_timing.launches == 2
    got = out.cpu().numpy()
    assert got.shape == (W, _lib.bias_stride(K)) and np.array_equal(got.view(np.uint64), timed.cpu().numpy().view(np.uint64))
    ref = bc.reference(before["mu"], before["pi_end"], before["A"], before["fcast"], 12, True)
    bc.check(_lib.unpack_bias(got, K), ref, bc.tolerance(ref, nrun, K, 12), "panel K=%d" % K)
    for n in _lib.DRAW_KEYS:
        assert np.array_equal(getattr(p, n).cpu().numpy(), before[n])
    with pytest.raises(_lib.HmcgError, match="keep_draws"):
        DevicePanel(Y, Tw, K, nrun, (12,), fut[:, 11:12], keep_draws=False).bias_moments()


def test_estimatewindows_bias_equals_the_file_route(inflation, tmp_path):
    """code/run_hmm.jl's windows for two end dates: BatchResult.bias from the device against bias_calcs.jl's route over the
    per-draw files saveresults writes; totalbias against the rounded forecast-error draws; the same bits when the draws are
    not kept."""
    from hmc_jl_amd import hmc
    y, dates = inflation
    dd = [dt.date.fromisoformat(d) for d in dates]
    ends = [200, 201]
    kw = dict(horizons=[12], D=3, burnin=300, Nrun=1500, series="official", bias_horizon=12)
    res = hmc.estimatewindows(y, dd, ends, keep_draws=True, **kw)
    b = res.bias
    assert (res.status == 0).all() and b.uncerbias.shape == b.totalbias.shape == (2,) and b.mean.shape == (2, 6) and b.cov.shape == (2, 6, 6)
    for w in range(2):
        hmc.saveresults(res.samples(w), res.opts[w], str(tmp_path))
    want = [dd[e - 1] for e in ends]
    d_f, unc_f, tot_f, mean_f, cov_f = hmc.calcbias(str(tmp_path), want, 12)
    d_d, unc_d, tot_d, mean_d, cov_d = hmc.calcbias(str(tmp_path), want, 12, result=res)
    assert d_f == d_d == [str(d) for d in want] and np.array_equal(unc_d, b.uncerbias) and np.array_equal(cov_d, b.cov)
    r = res._res
    ref = bc.reference(r["mu"], r["pi_end"], r["A"], r["fcast"], 12, True)
    tol = bc.tolerance(ref, 1500, 3, 12)
    bc.check({"uncbias": unc_d, "totalbias": tot_d, "mean": mean_d, "cov": cov_d}, ref, tol, "device")
    # the file route is an fp64 two-pass computation of the same shape: both lie within the bound of the reference
    bc.check({"uncbias": unc_f, "totalbias": tot_f, "mean": mean_f, "cov": cov_f}, ref, tol, "files")
    for k, a, c in (("uncbias", unc_f, unc_d), ("totalbias", tot_f, tot_d), ("mean", mean_f, mean_d), ("cov", cov_f, cov_d)):
        assert (np.abs(a - c) <= 2.0 * tol[k]).all(), k
    fe = np.round(r["fcast"][:, 1, :], 5)
    assert (np.abs(tot_d - fe.mean(axis=1)) <= 1500 * 2.0 ** -52 * np.abs(fe).max(axis=1)).all()
    assert np.isfinite(unc_d).all() and np.isfinite(tot_d).all()
    lean = hmc.estimatewindows(y, dd, ends, keep_draws=False, **kw)
    for k in ("uncerbias", "totalbias", "mean", "cov"):
        assert np.array_equal(getattr(lean.bias, k).view(np.uint64), getattr(b, k).view(np.uint64)), k
    with pytest.raises(ValueError):
        lean.samples(0)
