"""hmcg_chain_quantiles[_device] on the GPU: exact quantiles by selection.  The result of a selection is an element of its input,
so every comparison here is bit for bit (quantile_cases.check): lo, hi, g, count and nan against the numpy reference (a stable
sort on the order-preserving key), value against the ABI's rule applied to the device's own lo, hi and g, NaN positions
separately.  Shapes are the smallest at which a selection can go wrong: nd around a wave (64), a tile of the block (4096 draws),
the candidate buffer (4096 keys: at 4097 draws no early gather after pass 0) and a many-tile column; columns of different
distributions per block; dirty padding behind nd."""
import datetime as dt

import numpy as np
import pytest

import quantile_cases as qc
import stat_device_entry as sde

pytestmark = pytest.mark.gpu

S = 1024


def _device_quantiles(x, nd, probs, round5=True, timed=True):
    """The device entry over torch buffers (stat_device_entry.run): x (W, C, ld) with ld >= nd.  Both outputs carry a sentinel
    window before and after their block, checked there.  Returns the unpacked output."""
    return sde.run("chain_quantiles", dict(x=x, nd=nd, probs=probs, round5=round5), timed)


def _edge_cases():
    """Every nd edge with Q, W x C, the padding and the ROUND5 flag dealt round-robin, so that each of them meets small and large
    columns; the 2 x 64 grid only where the reference sort stays small."""
    shapes = ((1, 1), (3, 9), (2, 64))
    probs = ((0.5,), qc.PROBS3, qc.PROBS16)
    out = []
    for i, nd in enumerate(qc.ND_EDGES):
        for k in range(3):
            W, Cn = shapes[(i + k) % 3]
            if nd > 5000 and W * Cn > 27:
                W, Cn = 3, 9
            out.append((nd, probs[k], W, Cn, 37 * ((i + k) % 2), (i + k) % 3 != 1))
    return out


@pytest.mark.parametrize("nd,probs,W,Cn,pad,round5", _edge_cases())
def test_device_entry_against_reference(nd, probs, W, Cn, pad, round5):
    x = qc.panel(100 * nd + Cn + len(probs), W, Cn, nd, pad)
    got = _device_quantiles(x, nd, probs, round5)
    qc.check(got, qc.reference(x, probs, round5, nd), "nd=%d Q=%d W=%d C=%d pad=%d r5=%s" % (nd, len(probs), W, Cn, pad, round5))
    assert (got["nan"] == 0).all() and np.isfinite(got["value"]).all()          # the padding (NaN, -inf, 1e300) was never read


def _ramp(start, n):
    out = np.empty(n)
    out[0] = start
    for i in range(1, n):
        out[i] = np.nextafter(out[i - 1], np.inf)
    return out


def _directed():
    """name -> (columns (C, nd), probs, round5)."""
    rng = np.random.default_rng(5)
    sh = lambda v: rng.permutation(np.asarray(v, dtype=np.float64))
    tiny = np.finfo(float).tiny
    nd = 4097
    cases = {}
    cases["constant"] = (np.stack([np.full(nd, 1.0 / 3.0), np.full(nd, -0.0), np.full(nd, 1e4 + 1.0 / 3.0)]), qc.PROBS16, True)
    cases["two values"] = (np.stack([sh([1.0] * 2000 + [2.0] * 2097), sh([-5.5] * 4096 + [7.25]), sh([0.1] + [0.2] * 4096)]), qc.PROBS16, False)
    # 4097 neighbours (the lowest 8 mantissa bits and one carry), and 256 neighbours 17 times: only the last digit tells them apart
    cases["ulp ramp"] = (np.stack([sh(_ramp(1.5, nd)), sh(np.tile(_ramp(-2.75, 256), 17)[:nd]), sh(-_ramp(1e-3, nd))]), qc.PROBS16, False)
    low = np.float64(1.2345678)
    cases["lowest bit"] = (np.stack([sh(np.where(np.arange(nd) % 3 == 0, low, np.nextafter(low, 2.0))),
                                     sh(np.where(np.arange(nd) % 2 == 0, -low, np.nextafter(-low, -2.0)))]), qc.PROBS16, False)
    cases["zeros"] = (np.stack([np.array([0.0, -0.0, -0.0]), np.array([-0.0, 0.0, 1e-300]), np.array([-1e-9, 0.0, 1e-9])]), (0.0, 1.0, 0.5, 0.25), False)
    cases["zeros rounded"] = (np.stack([np.array([0.0, -0.0, -0.0]), np.array([-1e-9, 1e-9, -2e-6]), np.array([-4e-6, 4e-6, 6e-6])]), (0.0, 1.0, 0.5), True)
    cases["around zero"] = (np.stack([sh(np.concatenate([rng.standard_normal(nd - 3) * 1e-3, [0.0, -0.0, -0.0]])),
                                      sh(np.concatenate([-np.exp(rng.standard_normal(2000)), np.exp(rng.standard_normal(2097))]))]), qc.PROBS16, False)
    cases["subnormals"] = (np.stack([sh(np.arange(-2000, 2097) * 5e-324), sh(np.concatenate([_ramp(tiny / 4, 2048), -_ramp(tiny / 8, 2049)]))]),
                           qc.PROBS16, False)
    cases["infinities"] = (np.stack([sh([-np.inf] + list(rng.standard_normal(63)) + [np.inf]), sh([-np.inf] * 3 + [0.5, 1.5] + [np.nan] * 60),
                                     sh([np.inf] * 40 + [-np.inf] * 25)]), (0.0, 1.0, 0.6, 0.01, 0.99, 0.25), False)
    a, b, c = rng.standard_normal(nd), rng.standard_normal(nd), rng.standard_normal(nd)
    a[0], b[nd // 2], c[-1] = np.nan, np.nan, np.nan
    d = rng.standard_normal(nd)
    d[rng.random(nd) < 0.3] = np.nan
    cases["nans"] = (np.stack([a, b, c, d]), qc.PROBS16, True)
    cases["all nan"] = (np.stack([np.full(nd, np.nan), rng.standard_normal(nd), np.full(nd, np.nan)]), qc.PROBS3, True)
    one = np.full((2, 70), np.nan)
    one[0, 33], one[1, 69] = 2.5, -0.0
    cases["m = 1"] = (one, qc.PROBS16, False)
    # half in [1, 2), half in [1024, 2048): with an even count the median's two ranks lie in different top-digit buckets
    cases["bucket boundary"] = (np.stack([sh(np.concatenate([1.0 + rng.random(3000), 1024.0 + 1024.0 * rng.random(3000)])),
                                          sh(np.concatenate([-(1.0 + rng.random(3000)), 1.0 + rng.random(3000)]))]), (0.5, 0.25, 0.75, 0.4999, 0.5001), False)
    cases["heavy ties"] = (np.stack([sh(np.where(rng.random(50003) < 0.9, 1.0, rng.random(50003))),
                                     sh(np.where(rng.random(50003) < 0.9, 1.0, 1.0 - 1e-5 * rng.integers(0, 3, 50003)))]), qc.PROBS16, True)
    cases["clamp"] = (np.array([[qc.CLAMP_HI, qc.CLAMP_LO]]), (qc.CLAMP_P, 0.5, 0.0, 1.0), False)
    return cases


DIRECTED = _directed()


@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_directed_columns(name):
    cols, probs, round5 = DIRECTED[name]
    x = np.ascontiguousarray(cols)[None]                       # one window
    got = _device_quantiles(x, x.shape[2], probs, round5)
    ref = qc.reference(x, probs, round5)
    qc.check(got, ref, name)
    for k in ("lo", "hi", "value"):                            # through the bit pattern, the sign of a zero included
        ok = ~np.isnan(ref[k])
        assert np.array_equal(qc.bits(got[k])[ok], qc.bits(ref[k])[ok]), (name, k)
    if name == "zeros":
        assert np.signbit(got["lo"][0, 0, 0]) and not np.signbit(got["lo"][0, 0, 1])         # p = 0: -0.0; p = 1: +0.0
    if name == "zeros rounded":
        assert np.signbit(got["lo"][0, 1, 0]) and got["lo"][0, 1, 0] == 0.0                   # -2e-6 rounds to -0.0, below +0.0
    if name == "infinities":
        assert got["value"][0, 1, 0] == -np.inf and np.isnan(got["value"][0, 1, 2]) and got["lo"][0, 1, 2] == -np.inf
        assert got["value"][0, 0, 1] == np.inf and (got["count"][0] == [65, 5, 65]).all()
    if name == "all nan":
        assert (got["count"][0] == [0, 4097, 0]).all() and (got["nan"][0] == [4097, 0, 4097]).all()
        assert all(np.isnan(got[k][0, [0, 2]]).all() for k in qc.FIELDS) and np.isfinite(got["value"][0, 1]).all()
    if name == "m = 1":
        assert (got["count"] == 1).all() and (got["lo"][0, 0] == 2.5).all() and np.signbit(got["hi"][0, 1]).all()
    if name == "bucket boundary":
        assert got["lo"][0, 0, 0] < 2.0 and got["hi"][0, 0, 0] >= 1024.0 and got["lo"][0, 1, 0] < 0.0 < got["hi"][0, 1, 0]
    if name == "clamp":
        assert got["g"][0, 0, 0] == 0.25 and got["value"][0, 0, 0] == qc.CLAMP_HI and got["value"][0, 0, 1] == qc.CLAMP_HI


def test_host_entry_equals_device_entry_bit_for_bit(monkeypatch):
    """Both entries and every grouping of the host entry's columns give the same bits; two runs of either are bit-identical.
    27 columns: groups of 1 (27 uploads through a ring of 3), of 2 (the last one short), of 26 (26 + 1) and all at once."""
    from hmc_jl_amd import _lib
    W, Cn, nd = 3, 9, 2 * S + 17
    x = qc.panel(77, W, Cn, nd)
    keys = qc.FIELDS + ("count", "nan")
    same = lambda a, b: all(np.array_equal(np.ascontiguousarray(a[k]).view(np.int64), np.ascontiguousarray(b[k]).view(np.int64)) for k in keys)
    dev = _device_quantiles(x, nd, qc.PROBS16)
    assert same(dev, _device_quantiles(x, nd, qc.PROBS16, timed=False))
    qc.check(dev, qc.reference(x, qc.PROBS16), "device")
    tm = _lib.Timing()
    one = _lib.chain_quantiles(x, qc.PROBS16, timing=tm)
    assert tm.launches == 1 and tm.kernel_ms > 0.0 and tm.call_ms >= tm.kernel_ms
    assert same(one, dev)
    for cap, launches in ((1, 27), (2, 14), (26, 2)):
        monkeypatch.setenv("HMCG_CHUNK_COLS", str(cap))
        got = _lib.chain_quantiles(x, qc.PROBS16, timing=tm)
        assert tm.launches == launches and same(got, dev), cap
    monkeypatch.delenv("HMCG_CHUNK_COLS")
    assert same(_lib.chain_quantiles(x, qc.PROBS16), dev)
    # a padded host array, three probabilities and no rounding
    y = qc.panel(78, 1, 9, nd, 37)
    monkeypatch.setenv("HMCG_CHUNK_COLS", "2")
    host = _lib.chain_quantiles(y, qc.PROBS3, nd=nd, round5=False)
    monkeypatch.delenv("HMCG_CHUNK_COLS")
    assert same(host, _device_quantiles(y, nd, qc.PROBS3, False))
    qc.check(host, qc.reference(y, qc.PROBS3, False, nd), "host, padded")


@pytest.mark.parametrize("K,T,nrun", [(3, 200, 2 * S + 17)])
def test_device_panel_chain_quantiles(K, T, nrun):
    """DevicePanel.chain_quantiles on the draws `run` left in HBM, mu (C = K) and A (C = K^2), against the reference on the
    panel's own fetched draws; the draws are unchanged afterwards."""
    from hmc_jl_amd import _lib, synth
    from hmc_jl_amd.device import DevicePanel
    W = 3
    Y, Tw, fut = synth.generate_panel(W, T, K)
    p = DevicePanel(Y, Tw, K, nrun, (12,), fut[:, 11:12])
    p.run(burnin=20, timed=False)
    out = {v: p.chain_quantiles(v) for v in ("mu", "A")}          # enqueued behind the run on the library stream
    p.sync()
    before = {n: getattr(p, n).cpu().numpy() for n in _lib.DRAW_KEYS}
    assert (p.status.cpu().numpy() == 0).all()
    for v in ("mu", "A"):
        got = _lib.unpack_chain_quantiles(out[v]["q"].cpu().numpy(), out[v]["n"].cpu().numpy())
        assert got["value"].shape == (W, K if v == "mu" else K * K, 3) and (got["count"] == nrun).all()
        qc.check(got, qc.reference(before[v], (0.05, 0.5, 0.95)), "panel %s" % v)
    assert (got["lo"][:, :, 0] <= got["lo"][:, :, 1]).all() and (got["lo"][:, :, 1] <= got["lo"][:, :, 2]).all()
    whole = p.chain_quantiles("fcast", qc.PROBS16, timed=True, round5=False)
    assert p.last_timing.kernel_ms > 0.0 and p.last_timing.launches == 1 and whole["q"].shape == (W, 2, 16, 4)
    got = _lib.unpack_chain_quantiles(whole["q"].cpu().numpy(), whole["n"].cpu().numpy())
    qc.check(got, qc.reference(before["fcast"], qc.PROBS16, False), "panel fcast")
    for n in _lib.DRAW_KEYS:
        assert np.array_equal(getattr(p, n).cpu().numpy(), before[n])
    with pytest.raises(_lib.HmcgError, match="keep_draws"):
        DevicePanel(Y, Tw, K, nrun, (12,), fut[:, 11:12], keep_draws=False).chain_quantiles()
    with pytest.raises(ValueError, match="var must be"):
        p.chain_quantiles("x")


def test_estimatewindows_quantiles_equal_the_file_route(inflation, tmp_path):
    """code/run_hmm.jl's windows for two end dates with short chains: BatchResult.quantiles from the device against the reference
    on samples(w) and against hmc.calcquantiles over the per-draw files saveresults writes from it -- the same bits, since a
    cell read back is the rounded draw -- and the same bits again when the draws are not kept."""
    from hmc_jl_amd import hmc
    y, dates = inflation
    dd = [dt.date.fromisoformat(d) for d in dates]
    ends = [200, 201]
    kw = dict(horizons=[12], D=3, burnin=300, Nrun=1500, series="official", quantile_vars=("mu", "fcast"))
    res = hmc.estimatewindows(y, dd, ends, keep_draws=True, **kw)
    assert (res.status == 0).all() and set(res.quantiles) == {"mu", "fcast"} and res.autocorr is None
    for w in range(2):
        hmc.saveresults(res.samples(w), res.opts[w], str(tmp_path))
    want = [dd[e - 1] for e in ends]
    lean = hmc.estimatewindows(y, dd, ends, keep_draws=False, **kw)
    keys = qc.FIELDS + ("count", "nan")
    for var in ("mu", "fcast"):
        d_f, files = hmc.calcquantiles(str(tmp_path), want, var)
        d_d, devq = hmc.calcquantiles(str(tmp_path), want, var, result=res)
        assert d_f == d_d == [str(d) for d in want] and devq.columns == files.columns and devq.probs == (0.05, 0.5, 0.95)
        draws = np.stack([(res.samples(w).mu if var == "mu" else res.samples(w).forecasts).T for w in range(2)])      # (W, C, nd)
        ref = qc.reference(draws, (0.05, 0.5, 0.95), True)
        qc.check({k: getattr(devq, k) for k in keys}, ref, "estimatewindows %s" % var)
        qc.check({k: getattr(files, k) for k in keys}, ref, "files %s" % var)
        for k in keys:
            assert np.array_equal(getattr(devq, k), getattr(files, k), equal_nan=True), (var, k)
            assert np.array_equal(getattr(lean.quantiles[var], k), getattr(devq, k), equal_nan=True), (var, k)
        assert (devq.count == 1500).all()
    with pytest.raises(ValueError):
        lean.samples(0)


def test_order_statistic_lies_in_the_bin_of_the_binned_route():
    """The two features on the same draws, nd = 1024: the order statistic lo = x_(j) -- the (j + 1)-th smallest -- falls by the
    ABI's bin rule into the very bin hmc.chainquantiles reports for q = (j + 1) / 1024 from hmcg_chain_density's counts."""
    from hmc_jl_amd import _lib, hmc
    import density_cases as dc
    nd, B = 1024, 64
    x = qc.panel(9, 2, 9, nd)
    probs = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0, 1.0 / 3.0)
    got = _lib.chain_quantiles(x, probs)
    parts = _lib.chain_density(x, None, B)
    dens = hmc.ChainDensity("mu", ["c%d" % c for c in range(9)], (nd,), 1, parts)
    qs = [(qc.rank(p, nd)[0] + 1) / 1024.0 for p in probs]
    binned = hmc.chainquantiles(dens, qs)
    for w in range(2):
        for c in range(9):
            lo, hi = parts["range"][w, c]
            slots = dc.histogram(got["lo"][w, c], lo, hi, B)
            assert np.array_equal(slots, binned["bin"][w, c, 0]), (w, c, slots, binned["bin"][w, c, 0])
    assert got["lo"][..., 0].tolist() == parts["range"][..., 0].tolist() and got["lo"][..., 6].tolist() == parts["range"][..., 1].tolist()
