"""hmcg_mixture_moments[_device] on the GPU: pooled mean, variance, skewness and excess kurtosis over the draws of the predictive
law sum_k omega_k N(mu_k, sig2_k), omega = pi_end A^h, and its within- / between-draw split, from hand-made draws and from the
sampler's own.

Reference (mixmoments_cases.reference): np.longdouble on the same arrays, np.round(x, 5) with round5, two-pass and central about
the true mean.  Per-cell absolute tolerance (mixmoments_cases.tolerance, derived, not measured): first order in 2^-53 from
eps_omega = 2 K h u per weight, n-term sums about the pivot with R = max |mu - c|, and the propagation through the central-moment
polynomials and the divisions by var^1.5 and var^2.  NaN positions must match exactly.

Largest differences an MI355X run of this module showed, as |diff| / its bound: mean 0.74 in the offset case (8.5e-13 against
1.1e-12: one rounding of a value near 1e4), in the case table 0.029 (4.0e-16 against 1.4e-14; this and the next four at K = 6,
nd = 1, horizons (0, 1, 12), raw draws); variance 0.011 (4.5e-15 against 1.7e-11, K = 8, nd = 1, the eight horizons), among K = 4..7
0.0086 (K = 4, nd = 1, horizon 0); skewness 0.0030 (3.7e-16 against 1.2e-13); kurtosis 0.0011 (8.9e-16 against 1.5e-11); within
0.0087 (1.6e-15 against 1.3e-12); between 0.0005 (2.4e-15 against 6.5e-12, K = 3, nd = 2), among K = 4..7 0.0003 (K = 7, nd = 2);
draw_skewness 0.0024 (4.8e-16 against 1.3e-12, K = 3, nd = 1), among K = 4..7 0.0016 (K = 6, nd = 1); weight 0.16 (3.5e-16 against
2.5e-14, K = 3, nd = 1), among K = 4..7 0.13 (K = 6, nd = 1).  The bound is a worst case over every summation order, so two to three digits of
slack are its nature, not a sign of a loose derivation constant.  Mean weight against the predictive CDF at y = 1e6: 7.8e-16
against 4.5e-13.  Pooled mean at h = 12 against the mean of the sampler's forecast draws: 8.0e-15 against 2.4e-12 (K = 3),
1.1e-14 against 9.2e-12 (K = 8).  Identical draws: variance - within exactly 0."""
import datetime as dt

import numpy as np
import pytest

import mixmoments_cases as mc
import stat_device_entry as sde

pytestmark = pytest.mark.gpu

H8 = (12, 0, 3, 1, 12, 7, 2, 5)
HSETS = ((0,), (12,), (0, 1, 12), H8)
U = 2.0 ** -53


def _device_mix(mu, sig2, pi, A, hz, nd, round5=True, timed=True):
    """The device entry over torch buffers (stat_device_entry.run): arrays with leading dimension mu.shape[2] >= nd.  Returns
    the unpacked output and the raw [W][n_h][8] block; the sentinel windows before and after it are checked there."""
    return sde.run("mixture_moments", dict(mu=mu, sig2=sig2, pi=pi, A=A, hz=hz, nd=nd, round5=round5), timed)


def _cases():
    """K in {2, 3, 8} x every nd of the issue (around the 64-lane wave, the 256-draw tile and the 1024-draw slab), with the four
    horizon sets ((0,) runs with A = NULL), W in {1, 3}, nd_ld = nd or nd + 5 and round5 on / off dealt round-robin, then the
    corners the deal misses."""
    S = 1024                      # asserted equal to _lib.PRED_SLAB in the test
    out = []
    idx = 0
    for K in (2, 3, 8):
        for nd in (1, 2, 63, 65, 255, 257, S - 1, S, S + 1, 2 * S + 17):
            out.append((K, nd, (1, 3)[(idx // 2) % 2], HSETS[idx % 4], 5 * ((idx // 2) % 2), (idx // 3) % 2 == 0))
            idx += 1
    out += [(3, 2 * S + 17, 3, (0, 12), 5, True),           # the production form: several windows x several slabs, padded
            (3, 2 * S + 17, 3, H8, 5, True),
            (8, 2 * S + 17, 3, H8, 0, False),               # the widest build: K = 8 beside 8 x 9 accumulators
            (2, S + 1, 3, H8, 5, False),
            (8, S + 1, 3, (0,), 5, True),
            (3, 1, 1, (12,), 0, True),                      # nd = 1 at every kind of horizon set
            (8, 1, 3, H8, 5, True),
            (2, 1, 1, (0, 1, 12), 0, False),
            (8, 2, 1, (0, 1, 12), 5, True)]
    return out + _mid_k_cases()


NEW_KS = (4, 5, 6, 7)             # the K between the three above; each in both builds, NHC = 2 (n_h <= 2) and NHC = HMCG_MAXH


def _mid_k_cases():
    """K = 4..7 at the smallest sizes that still meet every edge: one and two draws, one over the wave, the tile and the slab;
    the four horizon sets in turn (five sizes per K: every K meets all four, (0,) with A = NULL and H8 among them), W, nd_ld and
    round5 dealt as above (tests/test_stat_coverage.py checks the deal)."""
    out = []
    idx = 0
    for K in NEW_KS:
        for nd in (1, 2, 65, 257, 1025):
            out.append((K, nd, (1, 3)[(idx // 2) % 2], HSETS[idx % 4], 5 * ((idx // 2) % 2), (idx // 3) % 2 == 0))
            idx += 1
    return out


@pytest.mark.parametrize("K,nd,W,hz,pad,round5", _cases())
def test_device_entry_against_reference(K, nd, W, hz, pad, round5):
    from hmc_jl_amd import _lib
    assert _lib.PRED_SLAB == 1024
    mu, sig2, pi, A = mc.make_draws(1000 * K + nd + 31 * len(hz), W, K, nd, pad, any(h > 0 for h in hz))
    ref = mc.reference(mu, sig2, pi, A, hz, round5, nd)
    got, raw = _device_mix(mu, sig2, pi, A, hz, nd, round5)
    assert np.isfinite(raw).all()
    if nd == 1:
        assert (got["between"] == 0.0).all() and not np.signbit(got["between"]).any()
    mc.check(got, ref, mc.tolerance(ref, nd, K, hz), "K=%d nd=%d W=%d hz=%s pad=%d r5=%s" % (K, nd, W, hz, pad, round5))
    if hz == H8:
        assert np.array_equal(raw[:, 0].view(np.uint64), raw[:, 4].view(np.uint64)), "the two horizons 12 differ"


def test_identical_draws():
    """Every draw equal to draw 0: a_d = a_0 through the same instructions, so `between` is exactly 0.0; the pooled variance is
    then the within-draw variance up to the bound."""
    K, nd, W = 3, 1100, 2
    hz = (0, 12)
    mu, sig2, pi, A = mc.make_draws(8, W, K, 1)
    rep = lambda a: np.repeat(a, nd, axis=-1)
    got, _ = _device_mix(rep(mu), rep(sig2), rep(pi), rep(A), hz, nd)
    assert (got["between"] == 0.0).all()
    ref = mc.reference(rep(mu), rep(sig2), rep(pi), rep(A), hz, True)
    tol = mc.tolerance(ref, nd, K, hz)
    mc.check(got, ref, tol, "identical", ("mean", "variance", "within"))
    gap = np.abs(got["variance"] - got["within"])
    print("identical draws: |variance - within| max %.3e, bound %.3e" % (gap.max(), (tol["variance"] + tol["within"]).min()))
    assert (gap <= tol["variance"] + tol["within"]).all()


def test_large_offset_costs_no_digits():
    """Means at 1e4 plus a spread of 1e-2: the derived tolerance scales with the spread about the pivot (R ~ 1e-2), not with the
    offset -- raw moments about 0 would lose every digit of the fourth moment here."""
    K, nd, W = 3, 1500, 2
    hz = (0, 12)
    mu, sig2, pi, A = mc.make_draws(9, W, K, nd)
    mu = 1e4 + 1e-2 * (mu - 2.0) / 3.0
    sig2 = 1e-4 * sig2
    ref = mc.reference(mu, sig2, pi, A, hz, False)
    tol = mc.tolerance(ref, nd, K, hz)
    assert tol["variance"].max() < 1e-13 and float(ref["variance"].min()) > 1e-5
    assert tol["skewness"].max() < 1e-8 and tol["kurtosis"].max() < 1e-8 and tol["between"].max() < 1e-13
    got, _ = _device_mix(mu, sig2, pi, A, hz, nd, False)
    mc.check(got, ref, tol, "offset 1e4")


def test_one_nan_mean_poisons_its_window_only():
    K, nd, W = 3, 1030, 2
    hz = (0, 12)
    mu, sig2, pi, A = mc.make_draws(10, W, K, nd)
    mu[0, 1, 1027] = np.nan
    got, _ = _device_mix(mu, sig2, pi, A, hz, nd)
    for k in mc.FIELDS[:-1]:
        assert np.isnan(got[k][0]).all() and np.isfinite(got[k][1]).all(), k
    assert np.isfinite(got["weight"]).all()
    ref = mc.reference(mu, sig2, pi, A, hz, True)
    mc.check(got, ref, mc.tolerance(ref, nd, K, hz), "one NaN")


def test_zero_variance_in_one_state():
    K, nd, W = 3, 1030, 2
    hz = (0, 12)
    mu, sig2, pi, A = mc.make_draws(11, W, K, nd)
    sig2[:, 0, :] = 0.0
    got, raw = _device_mix(mu, sig2, pi, A, hz, nd)
    assert np.isfinite(raw).all()
    ref = mc.reference(mu, sig2, pi, A, hz, True)
    mc.check(got, ref, mc.tolerance(ref, nd, K, hz), "zero variance")


def test_host_entry_equals_device_entry_bit_for_bit(monkeypatch):
    """One slab cut and one pivot for both entries and for every chunking of the host entry's upload: the same bits."""
    from hmc_jl_amd import _lib
    S = _lib.PRED_SLAB
    K, W, nd = 3, 2, 3 * S + 17
    hz = (12, 0, 3)
    mu, sig2, pi, A = mc.make_draws(77, W, K, nd)
    _, dev = _device_mix(mu, sig2, pi, A, hz, nd)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    tm = _lib.Timing()
    one = _lib.mixture_moments_host(mu, sig2, pi, A, hz, timing=tm)
    assert tm.launches == 2 and tm.kernel_ms > 0.0 and tm.call_ms >= tm.kernel_ms
    monkeypatch.setenv("HMCG_CHUNK_DRAWS", str(S + 476))         # no slab multiple: rounded up to 2 slabs -> 2 chunks
    two = _lib.mixture_moments_host(mu, sig2, pi, A, hz, timing=tm)
    assert tm.launches == 3
    monkeypatch.setenv("HMCG_CHUNK_DRAWS", "1")                  # one slab per chunk: 4 chunks through a ring of 3 buffers
    four = _lib.mixture_moments_host(mu, sig2, pi, A, hz, timing=tm)
    assert tm.launches == 5
    monkeypatch.delenv("HMCG_CHUNK_DRAWS")
    again = _lib.mixture_moments_host(mu, sig2, pi, A, hz)
    for o in (one, two, four, again):
        assert np.array_equal(bits(o), bits(dev))
    assert np.array_equal(bits(_device_mix(mu, sig2, pi, A, hz, nd, timed=False)[1]), bits(dev))
    ref = mc.reference(mu, sig2, pi, A, hz, True)
    mc.check(_lib.unpack_mixture_moments(four), ref, mc.tolerance(ref, nd, K, hz), "host, 4 chunks")
    # horizon 0 without A, chunked: it is neither needed nor uploaded
    monkeypatch.setenv("HMCG_CHUNK_DRAWS", "1")
    h0 = _lib.mixture_moments_host(mu, sig2, pi, None, (0,))
    monkeypatch.delenv("HMCG_CHUNK_DRAWS")
    _, d0 = _device_mix(mu, sig2, pi, None, (0,), nd)
    assert np.array_equal(bits(h0), bits(d0)) and np.array_equal(bits(d0[:, 0]), bits(dev[:, 1]))


def test_same_omega_as_the_predictive_feature():
    """`weight` is the draw mean of sum_k omega_k, and so is a predictive CDF at a grid point where every Phi is exactly 1
    (y = 1e6).  Both features build omega by the same expression; the two numbers then differ by their summations alone: per draw
    K terms added in either order, (K - 1) 2^-53 each; nd per-draw values added in either order and one division, (nd + 1) 2^-53
    each; all relative to sum_k omega_k <= 1.001 (rows of 5-digit cells sum to 1 +- K 5e-6, 13 factors).  No share for the h-step
    recurrence."""
    from hmc_jl_amd import _lib
    K, nd, W, h = 3, 2000, 2, 12
    mu, sig2, pi, A = mc.make_draws(12, W, K, nd)
    got, _ = _device_mix(mu, sig2, pi, A, (h,), nd)
    cdf = _lib.predictive_cdf_host(mu, sig2, pi, A, np.array([1e6]), (h,))
    bound = 2 * (nd + K) * U * 1.001
    diff = np.abs(cdf[:, 0, 0] - got["weight"][:, 0])
    print("mean weight, predictive vs mixture moments: max |diff| = %.3e, bound %.3e" % (diff.max(), bound))
    assert (diff <= bound).all() and (np.abs(got["weight"] - 1.0) < 1e-3).all()


@pytest.mark.parametrize("K,T,nrun", [(3, 200, 700), (8, 700, 200), (5, 300, 200)])
def test_device_panel_mixture_moments(K, T, nrun):
    """DevicePanel.mixture_moments on the draws `run` left in HBM (K = 8 / T = 700 runs the LDS-resident kernel, whose scratch
    shares the device context with the slab sums); the draws are unchanged afterwards.  With round5 off the pooled mean at h = 12
    is the draw mean of the sampler's own forecast draws, which come from another code path ((pi' A^h) . mu with A^h by repeated
    squaring).  Bound: both omega chains carry 2 K h u per weight, K weights against |mu| <= M, and each path a K-term dot
    product: (4 K^2 h + 2 K) u M per draw; the pooled mean normalises by sum s_d / n, 1 up to (h + 1) K u in exact arithmetic
    (doubled); numpy's mean n u M; and the bound of the pooled mean itself."""
    from hmc_jl_amd import _lib, synth
    from hmc_jl_amd.device import DevicePanel
    W, hz = 3, (0, 12)
    Y, Tw, fut = synth.generate_panel(W, T, K)
    p = DevicePanel(Y, Tw, K, nrun, (12,), fut[:, 11:12])
    p.run(burnin=20, timed=False)
    out = p.mixture_moments(hz)                              # enqueued behind the run on the library stream
    p.sync()
    before = {n: getattr(p, n).cpu().numpy() for n in _lib.DRAW_KEYS}
    assert (p.status.cpu().numpy() == 0).all()
    timed = p.mixture_moments(hz, timed=True)
    assert p.last_timing.kernel_ms > 0.0 and p.last_timing.launches == 2
    got = out.cpu().numpy()
    assert got.shape == (W, 2, _lib.MIX_STRIDE) and np.array_equal(got.view(np.uint64), timed.cpu().numpy().view(np.uint64))
    ref = mc.reference(before["mu"], before["sig2"], before["pi_end"], before["A"], hz, True)
    mc.check(_lib.unpack_mixture_moments(got), ref, mc.tolerance(ref, nrun, K, hz), "panel K=%d" % K)
    raw = p.mixture_moments((12,), timed=True, round5=False).cpu().numpy()
    rref = mc.reference(before["mu"], before["sig2"], before["pi_end"], before["A"], (12,), False)
    rtol = mc.tolerance(rref, nrun, K, (12,))
    mc.check(_lib.unpack_mixture_moments(raw), rref, rtol, "panel K=%d raw" % K)
    M = np.abs(before["mu"]).max(axis=(1, 2))
    bound = (4 * K * K * 12 + 2 * K + 2 * K * 13 + nrun) * U * M + rtol["mean"][:, 0]
    diff = np.abs(raw[:, 0, 0] - before["fcast"][:, 0, :].mean(axis=1))
    print("panel K=%d: pooled mean at h = 12 vs the mean of the forecast draws: max |diff| = %.3e, bound %.3e" % (K, diff.max(), bound[np.argmax(diff)]))
    assert (diff <= bound).all()
    for n in _lib.DRAW_KEYS:
        assert np.array_equal(getattr(p, n).cpu().numpy(), before[n])
    with pytest.raises(_lib.HmcgError, match="keep_draws"):
        DevicePanel(Y, Tw, K, nrun, (12,), fut[:, 11:12], keep_draws=False).mixture_moments()


def test_estimatewindows_moments_equal_the_file_route(inflation, tmp_path):
    """code/run_hmm.jl's windows for two end dates: BatchResult.moments from the device against hmc.calcmoments over the per-draw
    files saveresults writes, and against the reference; the same bits when the draws are not kept."""
    from hmc_jl_amd import hmc
    y, dates = inflation
    dd = [dt.date.fromisoformat(d) for d in dates]
    ends = [200, 201]
    hz = (0, 12)
    kw = dict(horizons=[12], D=3, burnin=300, Nrun=1500, series="official", moment_horizons=hz)
    res = hmc.estimatewindows(y, dd, ends, keep_draws=True, **kw)
    m = res.moments
    assert (res.status == 0).all() and m.horizons == hz and all(getattr(m, k).shape == (2, 2) for k in mc.FIELDS)
    for w in range(2):
        hmc.saveresults(res.samples(w), res.opts[w], str(tmp_path))
    want = [dd[e - 1] for e in ends]
    d_f, files = hmc.calcmoments(str(tmp_path), want, hz)
    d_d, devm = hmc.calcmoments(str(tmp_path), want, hz, result=res)
    assert d_f == d_d == [str(d) for d in want] and all(np.array_equal(devm[k], getattr(m, k)) for k in mc.FIELDS)
    r = res._res
    ref = mc.reference(r["mu"], r["sig2"], r["pi_end"], r["A"], hz, True)
    tol = mc.tolerance(ref, 1500, 3, hz)
    mc.check(devm, ref, tol, "device")
    # the file route is an fp64 computation of the same shape: both lie within the bound of the reference
    mc.check(files, ref, tol, "files")
    for k in mc.FIELDS:
        assert (np.abs(files[k] - devm[k]) <= 2.0 * tol[k]).all() and np.isfinite(devm[k]).all(), k
    lean = hmc.estimatewindows(y, dd, ends, keep_draws=False, **kw)
    for k in mc.FIELDS:
        assert np.array_equal(getattr(lean.moments, k).view(np.uint64), getattr(m, k).view(np.uint64)), k
    with pytest.raises(ValueError):
        lean.samples(0)
