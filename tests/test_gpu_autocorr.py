"""hmcg_chain_autocorr[_device] on the GPU: autocovariances up to a largest lag, Geyer's integrated autocorrelation time,
effective sample size, Monte-Carlo standard error and split-R-hat of one draw column, from hand-made chains and from the
sampler's own.

Reference (autocorr_cases.reference): a_d = x'_d - p as the fp64 subtraction of the ABI, every sum and acov in np.longdouble.
(a) acov, mean and variance within the per-cell absolute bounds of autocorr_cases.tolerance (derived in that module's
docstring, nothing measured): acov_l (2 n + 8) 2^-53 (A_l + M Q_l + (n - l) M^2) / n, mean (n + 3) 2^-53 R + 2^-53 |mean|, variance
(3 n + 7) 2^-52 R^2.  (b) tau, ess, mcse, pairs, truncated and rhat array_equal -- NaN positions included -- with the fp64
restatement of the ABI's derived block applied to the device's own acov, variance and (restated bit for bit) sums.  (c) on the
AR(1) chains pairs and truncated equal to those of the long-double reference.

Largest differences an MI355X run of this module showed, as |diff| / its bound: acov 0.049 (3.1e-15 against 8.9e-14, nd = 9, L = 8,
C = 64), below 0.004 at every nd >= 1023, below 0.001 on the AR(1) chains and on the sampler's own draws; mean 0.82 (9.1e-13 against 1.1e-12
in the column offset by 1e4 at nd = 2: half an ulp of the result, the one rounding of p + S1 / n, against 2^-53 |mean|), 0.5 at
nd = 3089, 0.004 on the sampler's draws; variance 0.024 (nd = 3).  The sums behind the bounds are worst cases over every summation
order and sign pattern, so one to three digits of slack at large n are their nature.  The derived block, rhat, mean and variance
from the restated sums, NaN positions, and pairs / truncated on the AR(1) chains: equal in every case."""
import datetime as dt

import numpy as np
import pytest

import autocorr_cases as ac
import stat_device_entry as sde

pytestmark = pytest.mark.gpu

S = ac.SLAB
CS = (1, 3, 9, 64)
BUDGET = 2e7           # long-double multiply-adds of one case's reference


def _device_autocorr(x, nd, L, round5=True, timed=True):
    """The device entry over torch buffers (stat_device_entry.run): x (W, C, ld) with ld >= nd.  Both outputs carry a sentinel
    window before and after their block, checked there.  Returns the unpacked output."""
    return sde.run("chain_autocorr", dict(x=x, nd=nd, L=L, round5=round5), timed)


def _cases():
    """nd = L + 1 for every lag edge (the lags of one thread end at multiples of 8, the split of the threads over lags and
    draws changes at L + 1 = 16, 32, ..), nd = 1 and 2, then every slab edge of nd x every lag edge that fits; C, W, the NaN
    padding and the ROUND5 flag dealt round-robin, C and W lowered where the long-double reference would take too long."""
    out = [(1, 0, 3, 1, 5, True), (2, 0, 9, 3, 0, False), (2, 1, 64, 1, 5, True)]
    for k, L in enumerate(ac.LAG_EDGES[1:]):
        out.append((L + 1, L, CS[k % 4], (1, 3)[k % 2], 5 * (k % 2), k % 3 != 0))
    for i, nd in enumerate((S - 1, S, S + 1, 2 * S + 17, 5 * S + 3)):
        for k, L in enumerate(ac.LAG_EDGES):
            if L > nd - 1:
                continue
            Cn, W = CS[(i + k) % 4], (1, 3)[(i + k // 2) % 2]
            while W * Cn * nd * (L + 1) > BUDGET and (Cn > 1 or W > 1):
                Cn, W = (CS[max(CS.index(Cn) - 1, 0)], W) if Cn > 1 else (Cn, 1)
            out.append((nd, L, Cn, W, 5 * ((i + k) % 2), (i + k) % 3 != 1))
    return out


@pytest.mark.parametrize("nd,L,Cn,W,pad,round5", _cases())
def test_device_entry_against_reference(nd, L, Cn, W, pad, round5):
    x = ac.make_case(1000 * L + nd + Cn, W, Cn, nd, pad)
    ref = ac.reference(x, L, round5, nd)
    got = _device_autocorr(x, nd, L, round5)
    label = "nd=%d L=%d C=%d W=%d pad=%d r5=%s" % (nd, L, Cn, W, pad, round5)
    ac.check(got, ref, x, round5, nd, label)
    if nd > 2 * L + 2 and nd >= 64:
        assert np.isfinite(got["acov"]).all() and np.isfinite(got["mean"]).all()          # the NaN padding was never read


def test_ar1_chains_pairs_and_truncation():
    """(c): on the AR(1) chains the device's pairs and truncated are those of the long-double reference.  That may be asked
    only where no reference pair sum P_k up to the stop lies within the acov error of zero: every |P_k| must exceed 1e-6
    (the acov bound is near 1e-11 relative there)."""
    x, ref = ac.ar1_suite()
    for w in range(x.shape[0]):
        for c in range(x.shape[1]):
            assert min(abs(P) for P in ref["P"][w][c]) > 1e-6
    got = _device_autocorr(x, x.shape[2], ac.AR1_LAGS, False)
    ac.check(got, ref, x, False, None, "ar1")
    assert np.array_equal(got["pairs"], ref["pairs"]) and np.array_equal(got["truncated"], ref["truncated"])
    assert not got["truncated"].any()
    want = np.array([(1 + phi) / (1 - phi) for phi in ac.AR1_PHIS])
    assert (np.abs(got["tau"][0] - want) <= 0.1 * want).all(), (got["tau"], want)
    assert (np.abs(got["rhat"] - 1.0) < 0.02).all()


def test_constant_column_nan_and_short_window():
    """A constant column: acov exactly 0, the derived block NaN, pairs 0.  A NaN at draw 0, mid-chain and in the last L draws:
    every output of that column NaN, pairs and truncated 0, the other columns untouched.  A lag window too short for a slowly
    mixing chain: truncated = 1."""
    nd, L = 2 * S + 17, 63
    x = ac.make_case(5, 2, 5, nd)
    x[:, 1, :] = 1e4 + 1.0 / 3.0
    clean = _device_autocorr(x, nd, L)
    assert (clean["acov"][:, 1] == 0.0).all() and (clean["variance"][:, 1] == 0.0).all() and (clean["pairs"][:, 1] == 0).all()
    for k in ("tau", "ess", "mcse", "rhat"):
        assert np.isnan(clean[k][:, 1]).all(), k
    assert not clean["truncated"][:, 1].any() and (clean["mean"][:, 1] == ac.round5(1e4 + 1.0 / 3.0)).all()
    ac.check(clean, ac.reference(x, L), x, True, None, "constant")
    for where in (0, nd // 2, nd - 5):
        y = x.copy()
        y[0, 2, where] = np.nan
        y[1, 0, where] = np.inf
        got = _device_autocorr(y, nd, L)
        for w, c in ((0, 2), (1, 0)):
            assert np.isnan(got["acov"][w, c]).all(), (where, w, c)
            for k in ("variance", "tau", "ess", "mcse", "rhat"):
                assert np.isnan(got[k][w, c]), (where, k)
            assert not np.isfinite(got["mean"][w, c]) and got["pairs"][w, c] == 0 and not got["truncated"][w, c]
        keep = np.ones((2, 5), dtype=bool)
        keep[0, 2] = keep[1, 0] = False
        for k in ("acov",) + ac.FIELDS:
            assert np.array_equal(got[k][keep], clean[k][keep], equal_nan=True), (where, k)
        ac.check(got, ac.reference(y, L), y, True, None, "nan at %d" % where)
    slow = ac.ar1(11, 0.99, 4 * S)[None, None, :]
    got = _device_autocorr(slow, 4 * S, 15, False)
    assert got["truncated"][0, 0] and got["pairs"][0, 0] == 8
    ac.check(got, ac.reference(slow, 15, False), slow, False, None, "short window")


def test_host_entry_equals_device_entry_bit_for_bit(monkeypatch):
    """One slab split and one pivot for both entries and for every chunking of the host entry's upload: the same bits.  L = 1024:
    the draws in front of a chunk span a whole one-slab chunk.  Two runs of either entry are bit-identical."""
    from hmc_jl_amd import _lib
    W, Cn, nd, L = 2, 3, 3 * S + 17, 1024
    x = ac.make_case(77, W, Cn, nd)
    keys = ("acov",) + ac.FIELDS
    bits = lambda d: [np.ascontiguousarray(d[k]).view(np.uint64) if d[k].dtype == np.float64 else d[k] for k in keys]
    same = lambda a, b: all(np.array_equal(p, q) for p, q in zip(bits(a), bits(b)))
    dev = _device_autocorr(x, nd, L)
    assert same(dev, _device_autocorr(x, nd, L, timed=False))
    tm = _lib.Timing()
    one = _lib.chain_autocorr(x, L, timing=tm)
    assert tm.launches == 2 and tm.kernel_ms > 0.0 and tm.call_ms >= tm.kernel_ms
    monkeypatch.setenv("HMCG_CHUNK_DRAWS", str(3 * S))          # 2 chunks
    three = _lib.chain_autocorr(x, L, timing=tm)
    assert tm.launches == 3
    monkeypatch.setenv("HMCG_CHUNK_DRAWS", str(S))              # one slab per chunk: 4 chunks through a ring of 3 buffers
    four = _lib.chain_autocorr(x, L, timing=tm)
    assert tm.launches == 5
    monkeypatch.delenv("HMCG_CHUNK_DRAWS")
    for o in (one, three, four, _lib.chain_autocorr(x, L)):
        assert same(o, dev)
    ac.check(four, ac.reference(x, L), x, True, None, "host, 4 chunks")
    # a padded host array, a short lag window and no rounding
    y = ac.make_case(78, 1, 9, nd, 7)
    monkeypatch.setenv("HMCG_CHUNK_DRAWS", str(S))
    host = _lib.chain_autocorr(y, 17, nd=nd, round5=False)
    monkeypatch.delenv("HMCG_CHUNK_DRAWS")
    assert same(host, _device_autocorr(y, nd, 17, False))


@pytest.mark.parametrize("K,T,nrun", [(3, 200, 2 * S + 17)])
def test_device_panel_chain_autocorr(K, T, nrun):
    """DevicePanel.chain_autocorr on the draws `run` left in HBM, mu (C = K) and A (C = K^2), equals the host entry on the
    panel's own downloaded draws bit for bit and the reference within the bounds; the draws are unchanged afterwards."""
    from hmc_jl_amd import _lib, synth
    from hmc_jl_amd.device import DevicePanel
    W = 3
    Y, Tw, fut = synth.generate_panel(W, T, K)
    p = DevicePanel(Y, Tw, K, nrun, (12,), fut[:, 11:12])
    p.run(burnin=20, timed=False)
    out = {v: p.chain_autocorr(v, 100) for v in ("mu", "A")}          # enqueued behind the run on the library stream
    p.sync()
    before = {n: getattr(p, n).cpu().numpy() for n in _lib.DRAW_KEYS}
    assert (p.status.cpu().numpy() == 0).all()
    for v in ("mu", "A"):
        got = _lib.unpack_chain_autocorr(out[v]["acov"].cpu().numpy(), out[v]["diag"].cpu().numpy())
        assert got["acov"].shape == (W, K if v == "mu" else K * K, 101)
        host = _lib.chain_autocorr(before[v], 100)
        for k in ("acov",) + ac.FIELDS:
            assert np.array_equal(got[k], host[k], equal_nan=True), (v, k)
        ac.check(got, ac.reference(before[v], 100), before[v], True, None, "panel %s" % v)
    assert (got["ess"][np.isfinite(got["ess"])] > 0).all()
    whole = p.chain_autocorr("sig2", timed=True, round5=False)
    assert p.last_timing.kernel_ms > 0.0 and p.last_timing.launches == 2 and whole["acov"].shape == (W, K, 256)
    for n in _lib.DRAW_KEYS:
        assert np.array_equal(getattr(p, n).cpu().numpy(), before[n])
    with pytest.raises(_lib.HmcgError, match="keep_draws"):
        DevicePanel(Y, Tw, K, nrun, (12,), fut[:, 11:12], keep_draws=False).chain_autocorr()
    with pytest.raises(ValueError, match="var must be"):
        p.chain_autocorr("x")


def test_estimatewindows_autocorr_equals_the_file_route(inflation, tmp_path):
    """code/run_hmm.jl's windows for two end dates: BatchResult.autocorr from the device against hmc.calcess over the per-draw
    files saveresults writes -- both within the bounds of the long-double reference -- and the same bits when the draws are
    not kept."""
    from hmc_jl_amd import hmc
    y, dates = inflation
    dd = [dt.date.fromisoformat(d) for d in dates]
    ends = [200, 201]
    kw = dict(horizons=[12], D=3, burnin=300, Nrun=1500, series="official", acf_vars=("mu", "sig2"), acf_lags=120)
    res = hmc.estimatewindows(y, dd, ends, keep_draws=True, **kw)
    assert (res.status == 0).all() and set(res.autocorr) == {"mu", "sig2"} and res.density is None
    for w in range(2):
        hmc.saveresults(res.samples(w), res.opts[w], str(tmp_path))
    want = [dd[e - 1] for e in ends]
    lean = hmc.estimatewindows(y, dd, ends, keep_draws=False, **kw)
    for var in ("mu", "sig2"):
        d_f, files = hmc.calcess(str(tmp_path), want, var, 120)
        d_d, devd = hmc.calcess(str(tmp_path), want, var, 120, result=res)
        assert d_f == d_d == [str(d) for d in want] and devd.columns == files.columns == ["state_1", "state_2", "state_3"]
        ref = ac.reference(res._res[var], 120)
        tol = ac.tolerance(ref)
        for obj, name in ((devd, "device"), (files, "files")):
            for k in ("acov", "mean", "variance"):
                diff = np.abs(getattr(obj, k).astype(ac.LD) - ref[k]).astype(np.float64)
                assert (diff <= tol[k]).all(), (var, name, k, float((diff / tol[k]).max()))
        ac.check({k: getattr(devd, k) for k in ("acov",) + ac.FIELDS}, ref, res._res[var], True, None, "estimatewindows %s" % var)
        for k in ("acov",) + ac.FIELDS:
            assert np.array_equal(getattr(lean.autocorr[var], k), getattr(devd, k), equal_nan=True), k
    with pytest.raises(ValueError):
        lean.samples(0)
