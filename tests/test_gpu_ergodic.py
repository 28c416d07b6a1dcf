"""hmcg_ergodic_moments[_device] on the GPU.  The per-draw columns are compared with the numpy restatement of the ABI's rule BIT
FOR BIT (ergodic_cases.columns: one rounded operation per step, nothing fused); n exactly; the pooled mean and variance within
the derived bound of the longdouble moments of the device's own columns (ergodic_cases.check_pooled).  Shapes are the smallest at
which the kernel can go wrong: nd around a wave (64), a tile (256) and a slab (1024), more than two slabs with a short last one,
every K = 2..8 (each its own instantiation), dirty padding behind nd, NaN diagonals throughout."""
import datetime as dt

import numpy as np
import pytest

import ergodic_cases as ec
import stat_device_entry as sde

pytestmark = pytest.mark.gpu

S = ec.SLAB


def _device_ergodic(mu, sig2, A, nd, round5=True, cols=True, timed=True):
    """The device entry over torch buffers (stat_device_entry.run): mu, sig2 (W, K, ld), A (W, K, K, ld) with ld >= nd.  Every
    output carries a sentinel window before and after its block, checked there, as is the padding of cols.  Returns (cols
    (W, C, ld) or None, out (W, C, 2), n (W, 2))."""
    return sde.run("ergodic_moments", dict(mu=mu, sig2=sig2, A=A, nd=nd, round5=round5, cols=cols), timed)


def _places(nd, W, turn):
    """Directed draws at draw 0 (window 1: its pivot is then the draw's, or zeros), at a slab's last draw, in the last partial
    slab and at the last draw; the kinds dealt in turn."""
    spots = [(1 % W, 0), (0, S - 1), (W - 1, S), (0, nd - 1), (W - 1, nd // 2)]
    seen, out = set(), []
    for i, (w, d) in enumerate(spots):
        if 0 <= d < nd and (w, d) not in seen:
            seen.add((w, d))
            out.append((w, d, ec.DIRECTED[(turn + i) % len(ec.DIRECTED)]))
    return out


@pytest.mark.parametrize("round5", [True, False])
@pytest.mark.parametrize("K", ec.KS)
def test_columns_equal_the_restatement_bit_for_bit(K, round5):
    """Every nd edge, two windows, nd_ld = nd + 5 with NaN and 1e300 behind nd: cols cell for cell, n, and the pooled moments."""
    for i, nd in enumerate(ec.ND):
        W = 2
        mu, sig2, A = ec.make_panel(1000 * K + nd, W, K, nd, 5, _places(nd, W, i + K))
        cols, out, n = _device_ergodic(mu, sig2, A, nd, round5)
        want = ec.panel_columns(mu, sig2, A, nd, round5)
        assert ec.same_cells(cols[:, :, :nd], want), (K, nd, round5, np.argwhere(ec.bits(cols[:, :, :nd]) != ec.bits(want))[:4])
        ec.check_pooled(out, n, cols[:, :, :nd], "K=%d nd=%d r5=%s" % (K, nd, round5))
        assert (n.sum(axis=1) == nd).all()


@pytest.mark.parametrize("K", [2, 3, 5, 8])
def test_directed_draws(K):
    """Every directed kind at draw 0 of window 0, at the last draw of window 1's first slab and as the last draw (a partial slab)
    of window 2: the columns are the restatement's, the draw is good or not as its kind says, and everything else is untouched."""
    nd, W = 2 * S + 3, 3
    for t, name in enumerate(ec.DIRECTED):
        placed = ((0, 0, name), (1, S - 1, name), (2, nd - 1, name))
        mu, sig2, A = ec.make_panel(50 * K + t, W, K, nd, 3, placed)
        cols, out, n = _device_ergodic(mu, sig2, A, nd, True)
        want = ec.panel_columns(mu, sig2, A, nd, True)
        assert ec.same_cells(cols[:, :, :nd], want), (K, name)
        for w, d, _ in placed:
            x = cols[w, :, d]
            assert np.isfinite(x).all() == ec.directed_good(name, K), (K, name, w, d, x)
            if name == "absorbing first":
                assert np.array_equal(x[:K], np.eye(K)[0]) and x[K] == np.inf
            if name == "absorbing last":
                assert x[2 * K - 1] == np.inf and not np.isfinite(x[:K]).all()
            if name == "transient":
                assert x[K - 1] == 0.0 and not np.signbit(x[K - 1])
            if name == "persistent":
                assert (x[K:2 * K] == 1.0 / 1e-5).all() and np.allclose(x[:K], 1.0 / K, rtol=1e-14, atol=0.0)
        ec.check_pooled(out, n, cols[:, :, :nd], "K=%d %s" % (K, name))          # n exactly: the draws the restatement finds good
        assert (n[:, 1] >= (0 if ec.directed_good(name, K) else 1)).all() and (n.sum(axis=1) == nd).all()
        if name == "nan diagonal":                   # ... and with a finite diagonal in every draw: the same bits
            B = np.where(np.isnan(A), 0.5, A)
            B[:, :, :, nd:] = A[:, :, :, nd:]
            c2, o2, n2 = _device_ergodic(mu, sig2, B, nd, True)
            assert ec.same_cells(c2, cols) and ec.same_cells(o2, out) and np.array_equal(n2, n)


def test_pooled_moments_at_the_edges():
    """good = 0, 1 and 2; draw 0 not good (pivot 0) under a large common offset; a window of identical draws (variance exactly
    0 in every column); a NaN in mu or sig2 in the middle of a slab."""
    K, nd, W = 3, S + 65, 3
    rng = np.random.default_rng(3)
    a_bad = ec.directed("absorbing first", K, rng)
    for good_draws in ((), (5,), (5, S + 3)):
        mu, sig2, A = ec.make_panel(11 + len(good_draws), W, K, nd)
        keep = {d: (A[:, :, :, d].copy(), mu[:, :, d].copy(), sig2[:, :, d].copy()) for d in good_draws}
        A[:, :, :, :] = a_bad[0].T[None, :, :, None]
        for d, (a, m, s) in keep.items():
            A[:, :, :, d], mu[:, :, d], sig2[:, :, d] = a, m, s
        cols, out, n = _device_ergodic(mu, sig2, A, nd, False)
        assert (n == [len(good_draws), nd - len(good_draws)]).all()
        ec.check_pooled(out, n, cols, "good=%d" % len(good_draws))
        if len(good_draws) == 0:
            assert np.isnan(out).all()
        if len(good_draws) == 1:
            assert np.isnan(out[:, :, 1]).all() and ec.same_cells(out[:, :, 0], cols[:, :, 5])
        if len(good_draws) == 2:
            assert np.isfinite(out).all()
    # draw 0 not good in windows 0 and 1 (window 1: mu near 1e4, so the columns sit 1e4 from the pivot 0); window 2: identical draws
    mu, sig2, A = ec.make_panel(21, W, K, nd, 0, ((0, 0, "absorbing last"), (1, 0, "nan mu"), (0, 300, "nan sig2"), (1, 301, "nan mu")))
    for arr in (mu, sig2, A):
        arr[2] = arr[2][..., 7:8]
    cols, out, n = _device_ergodic(mu, sig2, A, nd, False)     # unrounded: every generic draw is irreducible, hence good
    assert ec.same_cells(cols, ec.panel_columns(mu, sig2, A, nd, False))
    assert (n == [[nd - 2, 2], [nd - 2, 2], [nd, 0]]).all()
    ec.check_pooled(out, n, cols, "pivot 0")
    assert abs(out[1, 2 * K, 0] - 1e4) < 10.0 and (out[2, :, 1] == 0.0).all() and ec.same_cells(out[2, :, 0], cols[2, :, 0])


def test_entries_and_chunkings_give_the_same_bits(monkeypatch):
    """The device entry with and without cols, timed or not, the host entry with and without cols, and the host entry uploading
    one slab (4 chunks through a ring of 3) or two slabs (2 chunks) at a time: the same bits in out, n and cols."""
    from hmc_jl_amd import _lib
    K, W, nd = 4, 2, 3 * S + 3
    mu, sig2, A = ec.make_panel(91, W, K, nd, 0, _places(nd, W, 0))
    cols, out, n = _device_ergodic(mu, sig2, A, nd)
    assert ec.same_cells(cols, ec.panel_columns(mu, sig2, A, nd))
    ec.check_pooled(out, n, cols, "device")
    for kw in (dict(cols=False), dict(timed=False), dict(cols=False, timed=False)):
        c2, o2, n2 = _device_ergodic(mu, sig2, A, nd, **kw)
        assert ec.same_cells(o2, out) and np.array_equal(n2, n) and (c2 is None or ec.same_cells(c2, cols)), kw

    def host(with_cols, launches):
        tm = _lib.Timing()
        e = _lib.ergodic_moments(mu, sig2, A, cols=with_cols, timing=tm)
        assert tm.launches == launches and tm.kernel_ms > 0.0 and tm.call_ms >= tm.kernel_ms
        got = np.stack([np.concatenate([e["pi_" + k], e["dur_" + k], e["mean_" + k][:, None], e["variance_" + k][:, None]], axis=1)
                        for k in ("mean", "var")], axis=2)
        assert ec.same_cells(got, out) and np.array_equal(np.stack([e["good"], e["bad"]], axis=1), n), (with_cols, launches)
        assert ("cols" in e) == with_cols and (not with_cols or ec.same_cells(e["cols"], cols)), (with_cols, launches)

    for with_cols in (True, False):
        host(with_cols, 2)
        monkeypatch.setenv("HMCG_CHUNK_DRAWS", "1")
        host(with_cols, 5)
        monkeypatch.setenv("HMCG_CHUNK_DRAWS", str(S + 1))
        host(with_cols, 3)
        monkeypatch.delenv("HMCG_CHUNK_DRAWS")
    # a padded host array: the first nd draws of a longer one, the padding dirty
    pm, ps, pA = ec.make_panel(91, W, K, nd, 9, _places(nd, W, 0))
    e = _lib.ergodic_moments(pm, ps, pA, cols=True, nd=nd)
    assert ec.same_cells(e["cols"], cols) and np.array_equal(e["good"], n[:, 0])


@pytest.mark.parametrize("K,T,nrun", [(3, 200, 2 * S + 17)])
def test_device_panel_ergodic_feeds_the_chain_entries(K, T, nrun):
    """DevicePanel.ergodic on the draws `run` left in HBM: the columns are the restatement's on the panel's own fetched draws;
    handed to chain_quantiles as they are (x=), the medians are numpy's by the quantile rule on the same columns and the NaN
    counts are the NaN cells; chain_density and chain_autocorr take them too."""
    import quantile_cases as qc
    from hmc_jl_amd import _lib, synth
    from hmc_jl_amd.device import DevicePanel
    W = 3
    Y, Tw, fut = synth.generate_panel(W, T, K)
    p = DevicePanel(Y, Tw, K, nrun, (12,), fut[:, 11:12])
    p.run(burnin=20, timed=False)
    e = p.ergodic(cols=True)
    q = p.chain_quantiles(probs=(0.05, 0.5, 0.95), round5=False, x=e["cols"])
    dens = p.chain_density(x=e["cols"], round5=False)
    acf = p.chain_autocorr(x=e["cols"], lags=20, round5=False)
    lean = p.ergodic(timed=True)
    assert p.last_timing.kernel_ms > 0.0 and p.last_timing.launches == 2 and "cols" not in lean
    p.sync()
    draws = {v: getattr(p, v).cpu().numpy() for v in ("mu", "sig2", "A")}
    cols = e["cols"].cpu().numpy()
    assert cols.shape == (W, 2 * K + 2, nrun) and ec.same_cells(cols, ec.panel_columns(draws["mu"], draws["sig2"], draws["A"]))
    out, n = e["out"].cpu().numpy(), e["n"].cpu().numpy()
    ec.check_pooled(out, n, cols, "panel")
    assert ec.same_cells(lean["out"].cpu().numpy(), out) and np.array_equal(lean["n"].cpu().numpy(), n)
    got = _lib.unpack_chain_quantiles(q["q"].cpu().numpy(), q["n"].cpu().numpy())
    qc.check(got, qc.reference(cols, (0.05, 0.5, 0.95), False), "quantiles of the ergodic columns")
    assert np.array_equal(got["nan"], np.isnan(cols).sum(axis=2)) and (got["count"] + got["nan"] == nrun).all()
    fin = np.isfinite(cols).all(axis=(1, 2))
    slack = 2.0 ** -51 * (np.abs(got["lo"]) + np.abs(got["hi"]))[fin][:, :, 1]              # three roundings of lo + g (hi - lo)
    assert (np.abs(got["value"][fin][:, :, 1] - np.quantile(cols[fin], 0.5, axis=2)) <= slack).all() and fin.any()
    u = _lib.unpack_ergodic(out, n, K)
    assert np.allclose(u["pi_mean"].sum(axis=1)[n[:, 0] > 0], 1.0, atol=1e-12)
    assert dens["counts"].shape[:2] == (W, 2 * K + 2) and acf["acov"].shape == (W, 2 * K + 2, 21)
    with pytest.raises(ValueError, match="x must be"):
        p.chain_quantiles(x=e["cols"][:, :, :-1])
    with pytest.raises(_lib.HmcgError, match="keep_draws"):
        DevicePanel(Y, Tw, K, nrun, (12,), fut[:, 11:12], keep_draws=False).ergodic()


def test_estimatewindows_ergodic_equals_the_file_route(inflation, tmp_path):
    """code/run_hmm.jl's windows for two end dates with short chains: BatchResult.ergodic from the device against
    hmc.calcergodic over the per-draw files saveresults writes from the same run -- a cell read back is the rounded draw, so the
    good counts are equal and both sets of pooled moments lie within the derived bound of the longdouble moments of the files'
    own per-draw columns -- and the same bits when the draws are not kept."""
    from hmc_jl_amd import hmc
    y, dates = inflation
    dd = [dt.date.fromisoformat(d) for d in dates]
    ends = [200, 201]
    kw = dict(horizons=[12], D=3, burnin=300, Nrun=1500, series="official", ergodic=True)
    res = hmc.estimatewindows(y, dd, ends, keep_draws=True, **kw)
    assert (res.status == 0).all() and res.quantiles is None and set(res.ergodic) >= {"pi_mean", "dur_var", "mean_mean", "good"}
    for w in range(2):
        hmc.saveresults(res.samples(w), res.opts[w], str(tmp_path))
    want = [dd[e - 1] for e in ends]
    d_f, files = hmc.calcergodic(str(tmp_path), want, cols=True)
    d_d, devc = hmc.calcergodic(str(tmp_path), want, result=res)
    assert d_f == d_d == [str(d) for d in want]
    block = lambda e: np.stack([np.concatenate([e["pi_" + k], e["dur_" + k], e["mean_" + k][:, None], e["variance_" + k][:, None]], axis=1)
                                for k in ("mean", "var")], axis=2)
    counts = lambda e: np.stack([e["good"], e["bad"]], axis=1)
    assert np.array_equal(counts(devc), counts(files)) and (devc["good"] + devc["bad"] == 1500).all()
    ec.check_pooled(block(devc), counts(devc), files["cols"], "estimatewindows")
    ec.check_pooled(block(files), counts(files), files["cols"], "files")
    assert np.allclose(devc["pi_mean"].sum(axis=1), 1.0, atol=1e-12) and (devc["dur_mean"] >= 1.0).all()
    lean = hmc.estimatewindows(y, dd, ends, keep_draws=False, **kw)
    for k, v in res.ergodic.items():
        assert np.array_equal(lean.ergodic[k], v, equal_nan=True), k
    with pytest.raises(ValueError):
        lean.samples(0)
