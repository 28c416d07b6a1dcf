"""hmcg_chain_density[_device] on the GPU: binned counts of nested chain prefixes, their mean and variance and the running mean
of one draw column (plots/mcplots.jl's plotchain / plotchainmean, plots/timeseriesplots.jl's plot_mean / plot_var up to the
drawing), from hand-made draws and from the sampler's own.

Reference (density_cases.reference): the bin rule restated in numpy fp64 -- counts, below, above, nan and range are compared
EXACTLY -- and np.longdouble two-pass moments and running sums about the same pivot.  Per-cell absolute tolerances
(density_cases.tolerance, derived in that module's docstring, nothing measured): mean (n + 3) 2^-53 R + 2^-53 |mean|, variance
(3 n + 7) 2^-52 R^2, trace the mean bound with that point's n; R = max |x' - p| over the prefix.  NaN and inf positions must match
exactly; the four groups of every prefix sum to its cut.

Largest differences an MI355X run of this module showed, as |diff| / its bound: mean 0.82 (9.1e-13 against 1.1e-12 in the column
offset by 1e4: half an ulp of the result, the one rounding of p + S1 / n, against 2^-53 |mean|); trace 0.97 in one cell of the case C = 64, B = 64, nd = 63, stride 1 (the final rounding
can use up the whole 2^-53 |mean| term when the result lies just above a power of two), 0.82 in the offset column; variance 0.041 (4.5e-16 against 1.1e-14, nd = 3089, five cuts).
A running mean over 80 slabs (nd = 81 925; strides 9, 80 and 1): trace 0.81, 0.80, 0.82, mean 0.13, 0.52, 0.23.  On the sampler's own draws (K = 3,
2065 and 1500 draws): mean 0.015, variance 0.0001, trace 0.42.  The R terms of the bounds are worst cases over every summation
order, so one to two digits of slack there are their nature; the |mean| term is tight by construction.  Counts, slots, range and
NaN positions: equal in every case."""
import datetime as dt

import numpy as np
import pytest

import density_cases as dc
import stat_device_entry as sde

pytestmark = pytest.mark.gpu

CS = (1, 3, 9, 16, 64)
BS = (1, 2, 64, 512)


def _device_density(x, nd, cuts, bins, lo_hi=None, trace=(0, 1), round5=True, timed=True):
    """The device entry over torch buffers (stat_device_entry.run): x (W, C, ld) with ld >= nd.  Every output carries a sentinel
    window before and after its block, checked there.  Returns the unpacked output and the four raw blocks."""
    return sde.run("chain_density", dict(x=x, nd=nd, cuts=cuts, bins=bins, lo_hi=lo_hi, trace=trace, round5=round5), timed)


def _cases():
    """Every nd of the issue (around the 64-lane wave, the 256-draw tile and the 1024-draw slab) x every C; bins, W, nd_ld - nd,
    round5, the range kind (automatic / narrower than the data / hi == lo), the cut set and the trace kind dealt round-robin;
    then the corners the deal misses."""
    out = []
    for i, nd in enumerate(dc.ND):
        for k, Cn in enumerate(CS):
            idx = i * len(CS) + k
            out.append((Cn, BS[idx % 4], nd, (1, 3)[(i + k) % 2], 5 * ((idx // 3) % 2), idx % 3 != 1, (i + k // 2) % 3, (i + k) % 5, (i + 2 * k) % 3))
    S = dc.SLAB
    out += [(64, 512, 2 * S + 17, 3, 5, True, 0, 4, 2),        # five column groups x several pieces x several windows
            (64, 512, S + 1, 1, 0, False, 1, 3, 1),
            (3, 64, 2 * S + 17, 3, 5, True, 0, 4, 1),          # the production form: K = 3, 64 bins, nested cuts, a running mean
            (9, 512, 2 * S + 17, 3, 0, True, 1, 2, 2),         # the second timing shape
            (9, 1, 2 * S + 17, 3, 5, True, 2, 1, 1),
            (16, 2, 1, 1, 5, False, 0, 0, 1),
            (9, 64, 2, 3, 0, True, 2, 1, 1)]
    return out


@pytest.mark.parametrize("Cn,bins,nd,W,pad,round5,rkind,ckind,tkind", _cases())
def test_device_entry_against_reference(Cn, bins, nd, W, pad, round5, rkind, ckind, tkind):
    from hmc_jl_amd import _lib
    assert _lib.PRED_SLAB == dc.SLAB
    x = dc.make_case(100 * Cn + nd + 7 * bins, W, Cn, nd, pad, bins)
    cuts, trace = dc.cut_set(ckind, nd), dc.trace_set(tkind, nd)
    lo_hi = dc.given_range(rkind, dc.reference(x, cuts, bins, None, (0, 1), round5, nd), W, Cn) if rkind else None
    ref = dc.reference(x, cuts, bins, lo_hi, trace, round5, nd)
    got, _ = _device_density(x, nd, cuts, bins, lo_hi, trace, round5)
    label = "C=%d B=%d nd=%d W=%d pad=%d r5=%s range=%d cuts=%s trace=%s" % (Cn, bins, nd, W, pad, round5, rkind, cuts, trace)
    dc.check(got, ref, label)
    if pad:
        assert ref["nan"].sum() == got["nan"].sum()         # the NaN padding was never read (array_equal above says the same)
    if rkind == 1 and nd > 64:
        assert (got["below"] + got["above"]).sum() > 0      # the given range is narrower than the data


def test_constant_column_and_padding():
    """A column of identical values: variance exactly 0.0 at every cut, every draw in bin 0; a NaN-padded array of clean draws
    counts no NaN."""
    nd, W, Cn = 2 * dc.SLAB + 17, 2, 3
    x = np.full((W, Cn, nd + 5), np.nan)
    rng = np.random.default_rng(3)
    x[:, :, :nd] = rng.normal(1.0, 0.2, size=(W, Cn, nd))
    x[:, 1, :nd] = 1e4 + 1.0 / 3.0
    cuts = (2, dc.SLAB, nd)
    got, _ = _device_density(x, nd, cuts, 64, None, (nd, 1))
    assert (got["variance"][:, 1, :] == 0.0).all() and (got["nan"] == 0).all()
    assert (got["counts"][:, 1, :, 0] == np.array(cuts)).all() and (got["trace"][:, 1, :] == got["mean"][:, 1, :1]).all()
    dc.check(got, dc.reference(x, cuts, 64, None, (nd, 1), True, nd), "constant")
    one, _ = _device_density(x, 1, (1,), 8, None, (1, 1))
    assert np.isnan(one["variance"]).all() and (one["counts"][..., 0] == 1).all()


def test_host_entry_equals_device_entry_bit_for_bit(monkeypatch):
    """One piece list and one pivot for both entries and for every chunking of the host entry's upload: the same bits, with the
    automatic range (two upload passes) and with a given one; two runs of either entry are bit-identical."""
    from hmc_jl_amd import _lib
    S = _lib.PRED_SLAB
    W, Cn, nd, bins = 2, 9, 3 * S + 17, 64
    x = dc.make_case(77, W, Cn, nd, 0, bins)
    cuts, trace = (5, S, S + 300, 2 * S + 1, nd - 1), (nd // 7, 7)
    bits = lambda d: [np.ascontiguousarray(d[k]).view(np.uint64 if d[k].dtype == np.float64 else np.int64) for k in _lib.DENS_FIELDS]
    same = lambda a, b: all(np.array_equal(p, q) for p, q in zip(bits(a), bits(b)))
    ref_auto = dc.reference(x, cuts, bins, None, trace, True)
    for lo_hi in (None, dc.given_range(1, ref_auto, W, Cn)):
        dev, _ = _device_density(x, nd, cuts, bins, lo_hi, trace)
        again, _ = _device_density(x, nd, cuts, bins, lo_hi, trace, timed=False)
        assert same(dev, again)
        passes = 2 if lo_hi is None else 1
        tm = _lib.Timing()
        one = _lib.chain_density(x, cuts, bins, lo_hi, trace, timing=tm)
        assert tm.launches == passes + 2 and tm.kernel_ms > 0.0 and tm.call_ms >= tm.kernel_ms
        monkeypatch.setenv("HMCG_CHUNK_DRAWS", "2048")               # 2 chunks
        two = _lib.chain_density(x, cuts, bins, lo_hi, trace, timing=tm)
        assert tm.launches == 2 * passes + 2
        monkeypatch.setenv("HMCG_CHUNK_DRAWS", "1024")               # one slab per chunk: 4 chunks through a ring of 3 buffers
        four = _lib.chain_density(x, cuts, bins, lo_hi, trace, timing=tm)
        assert tm.launches == 4 * passes + 2
        monkeypatch.delenv("HMCG_CHUNK_DRAWS")
        for o in (one, two, four, _lib.chain_density(x, cuts, bins, lo_hi, trace)):
            assert same(o, dev)
        dc.check(four, dc.reference(x, cuts, bins, lo_hi, trace, True), "host, 4 chunks")
    # cuts and a running mean that end early: the chunks beyond them are not uploaded a second time
    monkeypatch.setenv("HMCG_CHUNK_DRAWS", "1024")
    tm = _lib.Timing()
    early = _lib.chain_density(x, (5, 700), bins, None, (100, 3), timing=tm)
    monkeypatch.delenv("HMCG_CHUNK_DRAWS")
    assert tm.launches == 4 + 1 + 2
    dev, _ = _device_density(x, nd, (5, 700), bins, None, (100, 3))
    assert same(early, dev)
    # a running mean that reaches beyond the last cut
    late, _ = _device_density(x, nd, (5,), bins, None, (nd, 1))
    dc.check(late, dc.reference(x, (5,), bins, None, (nd, 1), True), "trace beyond the last cut")


@pytest.mark.parametrize("stride,cuts", [(9, (5, 40 * dc.SLAB + 3)), (80, (80 * dc.SLAB + 5,)), (1, (7,))])
def test_running_mean_over_many_pieces(stride, cuts):
    """A running mean that spans 80 slabs -- more pieces than one trace of HMCG_DENS_MAXTRACE points at stride 1 can touch --
    with strides above 1, ending inside the last slab, and (stride 1) the longest trace the ABI allows, far beyond the only cut:
    the sum before each piece has to be there for every piece, not for the first 64 + HMCG_MAXH."""
    from hmc_jl_amd import _lib
    nd = 80 * dc.SLAB + 5
    x = dc.make_case(91, 1, 2, nd, 3, 16)
    x[0, 1, :nd] = 1e4 + 1e-2 * np.random.default_rng(92).standard_normal(nd)
    trace = (min((nd - 2) // stride, _lib.DENS_MAXTRACE), stride)
    assert trace[0] * stride > 74 * dc.SLAB or stride == 1
    got, _ = _device_density(x, nd, cuts, 16, None, trace)
    ref = dc.reference(x, cuts, 16, None, trace, True, nd)
    dc.check(got, ref, "long trace, stride %d" % stride)
    assert np.isfinite(got["trace"]).all() and not (got["trace"][0, :, -1] == got["trace"][0, :, 0]).any()
    host = _lib.chain_density(x[:, :, :nd], cuts, 16, None, trace)
    assert np.array_equal(host["trace"].view(np.uint64), got["trace"].view(np.uint64))


@pytest.mark.parametrize("K,T,nrun", [(3, 200, 2 * dc.SLAB + 17)])
def test_device_panel_chain_density(K, T, nrun):
    """DevicePanel.chain_density on the draws `run` left in HBM, mu (C = K) and A (C = K^2), against the reference applied to the
    panel's own downloaded draws; the draws are unchanged afterwards."""
    from hmc_jl_amd import _lib, synth
    from hmc_jl_amd.device import DevicePanel
    W = 3
    Y, Tw, fut = synth.generate_panel(W, T, K)
    p = DevicePanel(Y, Tw, K, nrun, (12,), fut[:, 11:12])
    p.run(burnin=20, timed=False)
    cuts, trace = (500, dc.SLAB, nrun), (200, 10)
    out = {v: p.chain_density(v, cuts, 32, None, trace) for v in ("mu", "A")}          # enqueued behind the run on the library stream
    p.sync()
    before = {n: getattr(p, n).cpu().numpy() for n in _lib.DRAW_KEYS}
    assert (p.status.cpu().numpy() == 0).all()
    for v in ("mu", "A"):
        o = {k: t.cpu().numpy() for k, t in out[v].items()}
        got = _lib.unpack_chain_density(o["range"], o["counts"], o["stats"], o["trace"])
        Cn = K if v == "mu" else K * K
        assert got["counts"].shape == (W, Cn, 3, 32)
        dc.check(got, dc.reference(before[v], cuts, 32, None, trace, True), "panel %s" % v)
    whole = p.chain_density("sig2", timed=True)
    assert p.last_timing.kernel_ms > 0.0 and p.last_timing.launches == 4
    assert (whole["counts"].cpu().numpy().sum(axis=3) == nrun).all() and whole["trace"].shape == (W, K, 0)
    lh = np.tile(np.array([0.0, 1.0]), (W, K, 1))
    given = p.chain_density("pi_end", (nrun,), 10, lh, timed=True, round5=False)
    o = {k: t.cpu().numpy() for k, t in given.items()}
    dc.check(_lib.unpack_chain_density(o["range"], o["counts"], o["stats"], o["trace"]),
             dc.reference(before["pi_end"], (nrun,), 10, lh, (0, 1), False), "panel pi_end")
    for n in _lib.DRAW_KEYS:
        assert np.array_equal(getattr(p, n).cpu().numpy(), before[n])
    with pytest.raises(_lib.HmcgError, match="keep_draws"):
        DevicePanel(Y, Tw, K, nrun, (12,), fut[:, 11:12], keep_draws=False).chain_density()
    with pytest.raises(ValueError, match="var must be"):
        p.chain_density("x")


def test_estimatewindows_density_equals_the_file_route(inflation, tmp_path):
    """code/run_hmm.jl's windows for two end dates: BatchResult.density from the device against hmc.calcchain over the per-draw
    files saveresults writes -- the counts, the range and the slots exactly, the moments within the bounds -- and against the
    reference; the same bits when the draws are not kept."""
    from hmc_jl_amd import _lib, hmc
    y, dates = inflation
    dd = [dt.date.fromisoformat(d) for d in dates]
    ends = [200, 201]
    cuts, bins, trace = (600, 1000, 1500), 48, (150, 10)
    kw = dict(horizons=[12], D=3, burnin=300, Nrun=1500, series="official", density_vars=("mu", "sig2"), density_cuts=cuts,
              density_bins=bins, density_trace=trace)
    res = hmc.estimatewindows(y, dd, ends, keep_draws=True, **kw)
    assert (res.status == 0).all() and set(res.density) == {"mu", "sig2"}
    for w in range(2):
        hmc.saveresults(res.samples(w), res.opts[w], str(tmp_path))
    want = [dd[e - 1] for e in ends]
    lean = hmc.estimatewindows(y, dd, ends, keep_draws=False, **kw)
    for var in ("mu", "sig2"):
        d_f, files = hmc.calcchain(str(tmp_path), want, var, cuts, bins, None, trace)
        d_d, devd = hmc.calcchain(str(tmp_path), want, var, cuts, bins, None, trace, result=res)
        assert d_f == d_d == [str(d) for d in want] and devd.columns == files.columns == ["state_1", "state_2", "state_3"]
        ref = dc.reference(res._res[var], cuts, bins, None, trace, True)
        g = {k: getattr(devd, k) for k in _lib.DENS_FIELDS}
        f = {k: getattr(files, k) for k in _lib.DENS_FIELDS}
        dc.check(g, ref, "device %s" % var)
        dc.check(f, ref, "files %s" % var)
        for k in dc.EXACT:
            assert np.array_equal(g[k], f[k]), k
        for k in _lib.DENS_FIELDS:
            a, b = getattr(lean.density[var], k), g[k]
            assert np.array_equal(a.view(np.int64), b.view(np.int64)), k
        q = hmc.chainquantiles(devd, (0.05, 0.95))
        assert (q["lo"][..., 0] <= devd.mean).all() and (devd.mean <= q["hi"][..., 1]).all()
    with pytest.raises(ValueError):
        lean.samples(0)

