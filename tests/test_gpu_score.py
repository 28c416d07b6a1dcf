"""hmcg_predictive_scores[_device] on the GPU: the continuous ranked probability score of the regime mixture's predictive law
against the realised value, its parts E|X - y| and E|X - X'|, the probability integral transform and the density, from hand-made
draws and from the sampler's own.

Reference and bounds (score_cases, derived there): the formulas of include/hmcg_score.h with erf and exp in float64 and every
sum, weight and product in long double; every field within its bound -- relative to E1 = e_abs and E2 = e_pair, whose terms are
all non-negative: tol1 E1, tol2 E2, tol1 E1 + tol2 E2 / 2 for crps, the CDF entry's bound for pit, tol1 times the mixture of
the components' peak densities for pdf.  The cases: K in {2, 3, 8} x used-draw counts 1, on both sides of the pair kernel's
tile edge (256 components), of one block's row share (512 components) and of the linear pass's slab (1 024 draws); strides 1, 2, 3;
padded arrays with NaN behind nd; rounding on and off; one, three and eight horizons; W in {1, 3}; realised values inside the
law, unknown, and 40 standard deviations out on either side.  Bits: two runs, both entries, the host entry forced to one and two
windows per group, equal horizons, identical windows; without rounding and thinning pit is hmcg_predictive_cdf_device's value
at yreal bit for bit, at horizons > 0 too, so the weights hold the siblings' bits.

What an MI355X run of this module showed, as the largest |device - ref| / bound per field and its case: crps and e_abs 0.016
(K = 2, 129 used draws, eight horizons), e_pair 0.011 (K = 3, one draw) and 0.002 at more than one draw (K = 5, 52 used draws:
the draw that straddles the tile edge), pit 0.0085 (K = 5, 52 used draws, seven horizons), pdf 0.0068 (K = 3, one draw); among
the K = 4..7 cases e_abs 0.013 (K = 4, 129 used draws, seven horizons), crps 0.009 (K = 5, 103 used draws), e_pair 0.0035 and
pdf 0.0023 (K = 4, one draw); on the inflation data (1 500 draws, horizons 0 and 12) the
device 0.0041 and the file route 0.0005 of the bound from the reference, 0.0023 of twice the bound from each other.
Measured at 460 windows x 250 000 draws, horizons (0, 12), default thinning (4 033 used draws), tools/score_bench.py: 156 ms at
K = 3 (3.44e10 pair terms, 2.20e11 /s) and 1 058 ms at K = 8 (2.28e11 /s) beside hmcg_predictive_cdf_device's 185 ms (3.02e11
Phi/s) and 700 ms (2.13e11 Phi/s) in the same session: 0.73 and 1.07 of its rate; the linear pass 0.6 % and 0.4 % of the call;
the pair kernel at its VALU issue, about 180 fp64 instructions a pair (113 VGPRs, four waves a SIMD).  One exact window, stride
1, 20 000 draws, K = 3: 23.9 ms for 1.81e9 pair terms."""
import datetime as dt

import numpy as np
import pytest

import fan_cases as fc
import score_cases as sc
import stat_device_entry as sde

pytestmark = pytest.mark.gpu

SENTINEL = sde.SENTINEL


def _device_scores(mu, sig2, pi, A, yreal, horizons, stride, nd, round5=True):
    """The device entry over torch buffers (stat_device_entry.run): arrays with leading dimension mu.shape[2] >= nd; out
    prefilled with a sentinel, framed by a sentinel window on either side."""
    return sde.run("predictive_scores", dict(mu=mu, sig2=sig2, pi=pi, A=A, yreal=yreal, horizons=horizons, stride=stride, nd=nd, round5=round5))


def _device_cdf(mu, sig2, pi, A, grid, horizons, nd, round5):
    return sde.run("predictive_cdf", dict(mu=mu, sig2=sig2, pi=pi, A=A, grid=grid, horizons=horizons, nd=nd, round5=round5))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _check(out, ref, bound, label):
    assert not (out == SENTINEL).any(), label
    worst = sc.worst_ratio(out, ref, bound)
    per = [sc.worst_ratio(out[..., i], ref[..., i], bound[..., i]) for i in range(5)]
    print("%s: max |device - ref| / bound = %.3g (%s)" % (label, worst, ", ".join("%s %.2g" % (n, v) for n, v in zip(sc.FIELDS, per))))
    assert worst <= 1.0, (label, out, ref, bound)
    return worst


def _pit_is_the_cdf_entry(mu, sig2, pi, A, y, horizons, nd, out):
    """With stride 1 and no rounding: hmcg_predictive_cdf_device with the realised values as its grid returns pit bit for bit."""
    from hmc_jl_amd import _lib
    W = mu.shape[0]
    known = [(j, w) for j in range(len(horizons)) for w in range(W) if not np.isnan(y[j, w])]
    if not known:
        return 0
    grid = np.array([y[j, w] for j, w in known])
    assert grid.size <= _lib.HMCG_MAXGRID
    cdf = _device_cdf(mu, sig2, pi, A, grid, horizons, nd, False)
    for g, (j, w) in enumerate(known):
        assert _same_bits(cdf[w, j, g], out[w, j, 3]), (w, j, cdf[w, j, g], out[w, j, 3])
    return len(known)


@pytest.mark.parametrize("K,n_u,stride,pad,round5,horizons,W", sc.GPU_CASES)
def test_device_entry_against_reference(K, n_u, stride, pad, round5, horizons, W):
    from hmc_jl_amd import _lib
    assert _lib.PRED_SLAB == sc.SLAB and _lib.SCORE_DRAWS_DEFAULT == sc.DRAWS_DEFAULT
    nd = sc.nd_of(n_u, stride)
    assert sc.thinning(nd, stride) == (stride, n_u)
    with_A = max(horizons) > 0
    mu, sig2, pi, A = fc.make_draws(3000 * K + n_u, W, K, nd, pad, with_A, 1.0 if n_u % 2 else 4.0)
    y = sc.make_yreal(mu, sig2, len(horizons), nd, n_u + K)
    ref, bound = sc.reference(mu, sig2, pi, A, y, horizons, stride, round5, nd)
    out = _device_scores(mu, sig2, pi, A, y, horizons, stride, nd, round5)
    _check(out, ref, bound, "K=%d n_u=%d stride=%d pad=%d round5=%s h=%s W=%d" % (K, n_u, stride, pad, round5, horizons, W))
    assert np.isfinite(out[..., 2]).all() and (out[..., 2] > 0.0).all() if n_u > 1 else True
    known = ~np.isnan(y.T)
    assert (out[..., 0][known] >= 0.0).all()
    far = known & (np.abs(y.T - 2.0) > 100.0)
    if far.any():
        # 40 standard deviations out: Phi is exactly 0 or 1 for every component, the score is the distance to the law
        up = y.T > 2.0
        wsum = np.where(up, out[..., 3], 0.0)
        assert (np.abs(wsum[far & up] - 1.0) < 1e-3).all() and (out[..., 3][far & ~up] == 0.0).all() and (out[..., 4][far] == 0.0).all()
        assert (out[..., 0][far] > 40.0).all()
    for a in range(len(horizons)):                                                        # equal horizons: e_pair in equal bits
        for b in range(a + 1, len(horizons)):
            if horizons[a] == horizons[b]:
                assert _same_bits(out[:, a, 2], out[:, b, 2])
    if stride == 1 and not round5:
        n = _pit_is_the_cdf_entry(mu, sig2, pi, A, y, horizons, nd, out)
        print("pit bit-equal to the CDF entry at %d points" % n)


def test_default_stride_case():
    """stride = 0 at nd = 8 209: stride 3, 2 737 used draws, K = 2 -- 22 tiles, 11 blocks, three slabs, 1.5e7 pair terms."""
    K, nd = sc.DEFAULT_CASE
    assert sc.thinning(nd, 0) == (3, 2737)
    mu, sig2, pi, A = fc.make_draws(4242, 1, K, nd, 0, True)
    horizons = (0, 12)
    y = np.array([[1.0], [6.5]])
    ref, bound = sc.reference(mu, sig2, pi, A, y, horizons, 0, True)
    out = _device_scores(mu, sig2, pi, A, y, horizons, 0, nd, True)
    _check(out, ref, bound, "default stride, nd=%d" % nd)
    assert _same_bits(out, _device_scores(mu, sig2, pi, A, y, horizons, 3, nd, True))


def test_runs_entries_groups_and_windows_give_the_same_bits(monkeypatch):
    """Two runs of the device entry, the host entry, the host entry forced to one and to two windows per upload group (a ring of
    3 buffers over 5 and 3 groups), with stride 1 and 3: the same bits; two identical windows and equal horizons score alike;
    without rounding pit is the CDF entry's value at horizons 0, 1 and 12 -- the weights hold the siblings' bits."""
    from hmc_jl_amd import _lib
    K, W, nd = 3, 5, 600
    horizons = (0, 1, 12, 1)
    mu, sig2, pi, A = fc.make_draws(88, W, K, nd, 0, True)
    for a in (mu, sig2, pi, A):
        a[4] = a[1]                                           # windows 1 and 4 are the same draws
    y = np.random.default_rng(3).normal(2.0, 3.0, size=(len(horizons), W))
    y[3], y[:, 4], y[2, 0] = y[1], y[:, 1], np.nan
    for stride, round5 in ((1, False), (3, True)):
        out = _device_scores(mu, sig2, pi, A, y, horizons, stride, nd, round5)
        assert _same_bits(_device_scores(mu, sig2, pi, A, y, horizons, stride, nd, round5), out)
        assert _same_bits(out[1], out[4]) and _same_bits(out[:, 1], out[:, 3])
        ref, bound = sc.reference(mu, sig2, pi, A, y, horizons, stride, round5)
        _check(out, ref, bound, "entries, stride %d" % stride)

        def host():
            tm = _lib.Timing()
            s = _lib.predictive_scores(mu, sig2, pi, A, y, horizons, stride, round5=round5, timing=tm)
            return np.stack([s[name] for name in _lib.SCORE_FIELDS], axis=-1), tm
        one, tm = host()
        assert tm.launches == 3 and tm.kernel_ms > 0.0 and tm.call_ms >= tm.kernel_ms
        monkeypatch.setenv("HMCG_SCORE_GROUP_WINDOWS", "1")
        five, tm = host()
        assert tm.launches == 15
        monkeypatch.setenv("HMCG_SCORE_GROUP_WINDOWS", "2")
        three, tm = host()
        assert tm.launches == 9
        monkeypatch.delenv("HMCG_SCORE_GROUP_WINDOWS")
        for got in (one, five, three):
            assert _same_bits(got, out)
        if stride == 1 and not round5:
            assert _pit_is_the_cdf_entry(mu, sig2, pi, A, y, horizons, nd, out) == 19
    # horizon 0 alone: A is neither needed nor uploaded
    h0 = _lib.predictive_scores(mu, sig2, pi, None, y[:1], (0,), 3)
    assert _same_bits(h0["crps"][:, 0], out[:, 0, 0]) and _same_bits(h0["e_pair"][:, 0], out[:, 0, 2])


def test_edge_inputs():
    """All draws hand-made.  Zero rounded variances in two components with equal means -- the 0 / 0 on and beside the diagonal
    that the one special case removes: crps, e_abs, e_pair and pit finite and within the bound (the density there is what IEEE
    gives: NaN).  A NaN mean under a zero weight: that window's whole row NaN, the window beside it untouched.  One draw.  All
    realised values unknown: e_pair alone, in the bits of a call that knows them."""
    K, nd, W = 2, 70, 2
    mu, sig2, pi, _ = fc.make_draws(5, W, K, nd, 0, False)
    mu[0, :, :20], sig2[0, 0, :20], sig2[0, 1, :20] = 1.37, 4e-6, 3e-6          # the variances round to 0
    y = np.array([[2.0, 2.0]])
    ref, bound = sc.reference(mu, sig2, pi, None, y, (0,), 1, True)
    out = _device_scores(mu, sig2, pi, None, y, (0,), 1, nd, True)
    assert np.isfinite(out[..., :4]).all() and np.isnan(out[0, 0, 4]) and np.isnan(ref[0, 0, 4]) and np.isfinite(out[1, 0, 4])
    _check(out, ref, bound, "zero variances")
    point = np.full((1, 2, 2), 1.37), np.full((1, 2, 2), 4e-6), np.full((1, 2, 2), 0.5)
    got = _device_scores(*point, None, np.array([[3.0]]), (0,), 1, 2, True)      # a point mass: |y - mu|, no spread (two draws: exact sums)
    assert got[0, 0, 0] == got[0, 0, 1] == 3.0 - 1.37 and got[0, 0, 2] == 0.0 and got[0, 0, 3] == 1.0
    # a NaN mean under a zero weight
    mu2, sig22, pi2, A2 = fc.make_draws(6, 2, 3, 300, 0, True)
    clean = _device_scores(mu2, sig22, pi2, A2, np.full((2, 2), 2.5), (0, 2), 1, 300, True)
    mu2[1, 1, 9], pi2[1, :, 9] = np.nan, (1.0, 0.0, 0.0)
    A2[1, :, :, 9] = np.eye(3)                                                               # the weight stays 0 at every horizon
    out = _device_scores(mu2, sig22, pi2, A2, np.full((2, 2), 2.5), (0, 2), 1, 300, True)
    assert np.isnan(out[1]).all() and _same_bits(out[0], clean[0]) and np.isfinite(clean).all()
    # one draw
    mu1, sig21, pi1, A1 = fc.make_draws(9, 1, 3, 1, 3, True)
    y1 = np.array([[2.0], [np.nan]])
    ref, bound = sc.reference(mu1, sig21, pi1, A1, y1, (0, 2), 0, True, 1)
    _check(_device_scores(mu1, sig21, pi1, A1, y1, (0, 2), 0, 1, True), ref, bound, "one draw")
    # all unknown
    mu3, sig23, pi3, A3 = fc.make_draws(10, 3, 3, 200, 0, True)
    known = _device_scores(mu3, sig23, pi3, A3, np.full((2, 3), 1.0), (0, 12), 2, 200, True)
    blind = _device_scores(mu3, sig23, pi3, A3, np.full((2, 3), np.nan), (0, 12), 2, 200, True)
    assert np.isnan(blind[..., [0, 1, 3, 4]]).all() and _same_bits(blind[..., 2], known[..., 2]) and (known[..., 2] > 0.0).all()


@pytest.mark.parametrize("K,T,nrun", [(3, 200, 700), (5, 300, 200)])
def test_device_panel_scores(K, T, nrun):
    """DevicePanel.scores on the draws `run` left in HBM (K = 3, T = 200, 700 draws; K = 5, T = 300, 200 draws: the
    sampler's own K = 5 draws, from the LDS-resident kernel, feed score_comp_kernel<5>; 3 windows) against the reference from the read-back draws;
    the draws are unchanged afterwards; a panel without draws refuses as `fan` does."""
    from hmc_jl_amd import _lib, synth
    from hmc_jl_amd.device import DevicePanel
    W = 3
    Y, Tw, fut = synth.generate_panel(W, T, K)
    p = DevicePanel(Y, Tw, K, nrun, (12,), fut[:, 11:12])
    p.run(burnin=20, timed=False)
    horizons = (0, 12)
    y = np.stack([Y[np.arange(W), Tw - 1], fut[:, 11]])
    y[1, 2] = np.nan
    s = p.scores(horizons, y, stride=1)                        # enqueued behind the run on the library stream
    p.sync()
    before = {n: getattr(p, n).cpu().numpy() for n in _lib.DRAW_KEYS}
    assert (p.status.cpu().numpy() == 0).all()
    timed = p.scores(horizons, y, stride=1, timed=True)
    assert p.last_timing.kernel_ms > 0.0 and p.last_timing.launches == 3
    out = s.cpu().numpy()
    assert _same_bits(out, timed.cpu().numpy())
    ref, bound = sc.reference(before["mu"], before["sig2"], before["pi_end"], before["A"], y, horizons, 1, True)
    _check(out, ref, bound, "panel")
    blind = p.scores(horizons)                                 # no realised values: the sharpness alone; default thinning = every draw
    p.sync()
    assert _same_bits(blind.cpu().numpy()[..., 2], out[..., 2]) and np.isnan(blind.cpu().numpy()[..., 0]).all()
    for n in _lib.DRAW_KEYS:
        assert np.array_equal(getattr(p, n).cpu().numpy(), before[n])
    with pytest.raises(_lib.HmcgError, match="keep_draws"):
        DevicePanel(Y, Tw, K, nrun, (12,), fut[:, 11:12], keep_draws=False).scores((0,))


def test_estimatewindows_scores_against_the_file_route(inflation, tmp_path):
    """code/run_hmm.jl's windows for two end dates: BatchResult.scores from the device against hmc.calcscores over the per-draw
    files saveresults writes.  Allowance for the five-decimal cells: a cell is off its draw by at most the half-unit 5e-6, but
    the device rounds every draw to its cell's value before use (HMCG_SCORE_ROUND5: rint(x * 1e5) / 1e5, the writer's rounding),
    so both routes score the same doubles and the half-unit does not enter: each is held to the bound against the long-double
    reference on the rounded draws, hence to twice the bound against the other.  The realised values are the series' own; the
    same bits when the draws are not kept; NaN where end + 12 lies past the series."""
    from hmc_jl_amd import _lib, hmc
    y, dates = inflation
    dd = [dt.date.fromisoformat(d) for d in dates]
    ends = [200, 201]
    horizons = (0, 12)
    kw = dict(horizons=[12], D=3, burnin=300, Nrun=1500, series="official", score_horizons=horizons)
    res = hmc.estimatewindows(y, dd, ends, keep_draws=True, **kw)
    s = res.scores
    assert (res.status == 0).all() and s["crps"].shape == (2, 2) and s["horizons"] == horizons and s["stride"] == 0
    yr = np.array([[y[e - 1 + h] for h in horizons] for e in ends])
    assert np.array_equal(s["yreal"], yr) and np.isfinite(s["crps"]).all() and (s["crps"] > 0.0).all()
    for w in range(2):
        hmc.saveresults(res.samples(w), res.opts[w], str(tmp_path))
    want = [dd[e - 1] for e in ends]
    d_f, s_f = hmc.calcscores(str(tmp_path), want, horizons, yr)
    d_d, s_d = hmc.calcscores(str(tmp_path), want, horizons, None, result=res)
    assert d_f == d_d == [str(d) for d in want] and _same_bits(s_d["crps"], s["crps"])
    r = res._res
    ref, bound = sc.reference(r["mu"], r["sig2"], r["pi_end"], r["A"], yr.T, horizons, 0, True)
    dev = np.stack([s[name] for name in _lib.SCORE_FIELDS], axis=-1)
    fil = np.stack([s_f[name] for name in _lib.SCORE_FIELDS], axis=-1)
    _check(dev, ref, bound, "estimatewindows, device")
    _check(fil, ref, bound, "estimatewindows, files")
    gap = np.abs(dev - fil) / (2.0 * bound)
    print("device vs file route: max |device - files| / (2 bound) = %.3g; crps %s" % (float(gap.max()), dev[..., 0].tolist()))
    assert (gap <= 1.0).all()
    sm = hmc.scoresummary(s)
    assert list(sm["count"]) == [2, 2] and sm["mean_crps"][0] == (s["crps"][0, 0] + s["crps"][1, 0]) / 2
    lean = hmc.estimatewindows(y, dd, ends, keep_draws=False, **kw)
    assert all(_same_bits(lean.scores[name], s[name]) for name in _lib.SCORE_FIELDS)
    with pytest.raises(ValueError):
        lean.samples(0)
    short = hmc.estimatewindows(y[:205], dd[:205], ends, keep_draws=False, **kw)           # end + 12 lies past the series
    assert np.isnan(short.scores["yreal"][:, 1]).all() and np.isnan(short.scores["crps"][:, 1]).all()
    assert _same_bits(short.scores["e_pair"], s["e_pair"]) and _same_bits(short.scores["crps"][:, 0], s["crps"][:, 0])
