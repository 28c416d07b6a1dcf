"""hmcg_predictive_quantiles[_device] on the GPU: quantiles of the regime mixture's predictive law (median, forecast bands,
value at risk) by grid refinement, from hand-made draws and from the sampler's own.

Reference (fan_cases.reference): the algorithm of include/hmcg_fan.h in float64 numpy with math.erfc.  The device is not asked
for the reference's bits beyond the range pass -- a cell choice may legitimately differ where two computed F differ by
rounding -- but for what a quantile must satisfy, judged by a long-double CDF (fan_cases.check_block; bounds derived there):
lo <= q <= hi, the bracket width (hi0 - lo0) / (128 * 32^(R - 1)) within 8 R ulps of the range's magnitude,
|F_ld(q) - p| <= B + 4 tolF, F_ld(lo) <= p + tolF, F_ld(hi) >= p - tolF.  `range` is asked bit for bit.  Flags must be the
reference's wherever the reference's own decision has a margin: an item whose reference values put p within tolF of Fhi, or
Fhi - Flo within 2 tolF of 0, may be flagged either way (no such item arises unless p is unreachable or the bracket has
collapsed below the resolution of F, rounds = 10).  Without round5 the returned lo and hi, handed to hmcg_predictive_cdf_device
as its grid, give Flo and Fhi back bit for bit.

What an MI355X run of this module showed: the largest |F_ld(q) - p| / (B + 4 tolF) 0.656 on the hand-made draws (K = 2, one
draw, one round; in the case table 0.404 at K = 5, one draw, two rounds, then 0.335 at K = 3 and 0.323 at K = 6, one draw each;
0.143 at K = 7, nd = 65; below 0.1 at nd = 1025 for every K) and 0.923 on the inflation data (nd = 1500, 4 rounds, the device and the file route alike: B is most of the
bound there); every bracket the restatement's except 2 of 45 and 3 of 48 at rounds = 10, where a step is two ulps of y; the
largest |q - q_ref| 4.6e-10 (K = 4, nd = 1025, one round: a bracket of (hi0 - lo0) / 128) and 1.1e-10 (K = 8, two rounds), every
bracket of the K = 4..7 cases the restatement's; the device and the file route 4.4e-16 apart on the inflation data."""
import datetime as dt

import numpy as np
import pytest

import fan_cases as fc
import predictive_cases as pc
import stat_device_entry as sde

pytestmark = pytest.mark.gpu

SENTINEL = sde.SENTINEL


def _device_fan(mu, sig2, pi, A, probs, horizons, rounds, nd, round5=True):
    """The device entry over torch buffers (stat_device_entry.run): arrays with leading dimension mu.shape[2] >= nd; outputs
    prefilled with a sentinel, framed by a sentinel window on either side."""
    return sde.run("predictive_quantiles", dict(mu=mu, sig2=sig2, pi=pi, A=A, probs=probs, horizons=horizons, rounds=rounds, nd=nd, round5=round5))


def _device_cdf(mu, sig2, pi, A, grid, horizons, nd, round5):
    return sde.run("predictive_cdf", dict(mu=mu, sig2=sig2, pi=pi, A=A, grid=grid, horizons=horizons, nd=nd, round5=round5))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b)


_flags_agree = sde.flags_agree             # flags equal to the reference's wherever its decision has a margin (module docstring)


def _cases():
    """K in {2, 3, 8} x nd around the tile (64) and the slab (1024), with n_p in {1, 5, 16}, rounds in {1, 2, 4, 10}, horizons (0,)
    with A = NULL or (0, 1, 12), W in {1, 3}, nd_ld = nd or nd + 5 and round5 on / off dealt round-robin (the strides 3, 4, 2 and
    the 6 sizes per K walk every pairing of n_p and rounds); then the corners the deal misses."""
    S = 1024                      # asserted equal to _lib.PRED_SLAB in the test
    nps = (fc.PROBS16[7:8], fc.PROBS5, fc.PROBS16)
    Rs = (1, 2, 4, 10)
    out = []
    idx = 0
    for K in (2, 3, 8):
        for nd in (1, 63, 65, S - 1, S + 1, 2 * S + 17):
            probs, R = nps[idx % 3], Rs[idx % 4]
            W = 3 if nd <= 65 else 1
            if nd > 2 * S and len(probs) == 16:               # the reference's cost: the many-probability, many-round pairings
                probs, R = (fc.PROBS5, R) if K == 8 else (probs, min(R, 2))      # stay on the sizes below two slabs
            out.append((K, nd, W, (0,) if idx % 2 == 0 else (0, 1, 12), probs, R, 5 * ((idx // 2) % 2), (idx // 3) % 2 == 0))
            idx += 1
    out += [(3, 2 * S + 17, 1, (0,), fc.PROBS5, 4, 5, True),             # the production form across slabs, padded
            (2, S + 1, 3, (12, 0), fc.PROBS16[7:8], 10, 0, False),       # several windows x several slabs, horizons in another order
            (3, 65, 3, fc.H8, fc.PROBS5, 4, 5, True),                    # HMCG_MAXH horizons, two of them equal
            (8, 65, 1, (0, 1, 2, 3, 5, 8, 12, 40), fc.PROBS16, 2, 0, False),     # the largest LDS tile, 3 968 items: 31 blocks of them
            (3, 63, 3, (0,), fc.PROBS16, 10, 0, False)]                  # the collapse of the bracket at every probability
    return out + _mid_k_cases(nps)


NEW_KS = (4, 5, 6, 7)             # the K between the three above: other staging remainders, LDS offsets and unrollings


def _mid_k_cases(nps):
    """K = 4..7 at the smallest sizes that still meet every edge: one draw, one over the 64-draw tile, one over the slab, with
    the three probability sets, one or two rounds, horizons (0,) with A = NULL or (0, 1, 12), nd_ld = nd or nd + 5 and round5
    on / off dealt so that every K meets each (tests/test_stat_coverage.py checks the deal)."""
    out = []
    idx = 0
    for K in NEW_KS:
        for nd in (1, 65, 1025):
            out.append((K, nd, 3 if nd <= 65 else 1, (0,) if (idx // 2) % 2 == 0 else (0, 1, 12), nps[idx % 3], (1, 2)[idx % 2],
                        5 * ((idx + idx // 3) % 2), ((idx + 1) // 2) % 2 == 0))
            idx += 1
    return out


@pytest.mark.parametrize("K,nd,W,horizons,probs,rounds,pad,round5", _cases())
def test_device_entry_against_reference(K, nd, W, horizons, probs, rounds, pad, round5):
    from hmc_jl_amd import _lib
    assert _lib.PRED_SLAB == 1024
    with_A = max(horizons) > 0
    mu, sig2, pi, A = fc.make_draws(2000 * K + nd + len(probs), W, K, nd, pad, with_A, 1.0 if nd % 2 else 4.0)
    e_out, e_rng, e_flag = fc.reference(mu, sig2, pi, A, probs, horizons, rounds, round5, nd)
    out, rng, flag = _device_fan(mu, sig2, pi, A, probs, horizons, rounds, nd, round5)
    assert _same_bits(rng, e_rng), (rng, e_rng)
    assert not (out == SENTINEL).any() and not (flag == -7).any()
    tol = fc.tolF(nd, K, horizons)
    ok, shaky = _flags_agree(flag, e_flag, e_out, probs, tol)
    assert ok, (flag, e_flag)
    worst = fc.check_block(out, rng, flag, probs, horizons, rounds, nd, K, fc.judge(mu, sig2, pi, A, horizons, round5, nd), "device")
    moved = int((out[..., 1] != e_out[..., 1]).sum())
    print("K=%d nd=%d W=%d h=%s n_p=%d R=%d pad=%d round5=%s: max |F_ld(q) - p| / (B + 4 tolF) = %.3g; flags %s, %d without margin; "
          "%d of %d brackets differ from the reference's; max |q - q_ref| = %.3e"
          % (K, nd, W, horizons, len(probs), rounds, pad, round5, worst, np.unique(flag), shaky, moved, flag.size,
             float(np.nanmax(np.abs(out[..., 0] - e_out[..., 0])))))
    # equal horizons, equal bits
    for a in range(len(horizons)):
        for b in range(a + 1, len(horizons)):
            if horizons[a] == horizons[b]:
                assert _same_bits(out[:, a], out[:, b]) and np.array_equal(flag[:, a], flag[:, b])
    if not round5:
        # the CDF entry at the returned bracket ends: the same bits
        grid = np.concatenate([out[..., 1].reshape(-1), out[..., 2].reshape(-1)])
        assert grid.size <= _lib.HMCG_MAXGRID
        cdf = _device_cdf(mu, sig2, pi, A, grid, horizons, nd, False)
        n = out[..., 1].size
        idx = np.arange(n).reshape(out.shape[:3])
        for w in range(W):
            for j in range(len(horizons)):
                assert _same_bits(cdf[w, j, idx[w, j]], out[w, j, :, 3]), (w, j, "Flo")
                assert _same_bits(cdf[w, j, n + idx[w, j]], out[w, j, :, 4]), (w, j, "Fhi")


def test_edge_inputs():
    """No special-casing, and the edge inputs end as the restatement says (test_fan.test_reference_edge_inputs): a NaN mean under
    a zero weight -- flag NAN and a NaN quantile for that window, the other window untouched, the range ignoring the NaN; a zero
    rounded variance -- a jump the bracket closes on; weights rounded to sum below p = 1 - 1e-6 -- UNREACHED with q = hi0 where
    round 1's last cell still climbs, FLAT once Phi has saturated below hi0; a one-draw window."""
    K, nd, W = 2, 70, 2
    mu, sig2, pi, _ = fc.make_draws(5, W, K, nd, 0, False)
    mu[1, 1, 9], pi[1, 0, 9], pi[1, 1, 9] = np.nan, 1.0, 0.0
    args = ((0.16, 0.5), (0,), 3, True)
    e_out, e_rng, e_flag = fc.reference(mu, sig2, pi, None, *args)
    out, rng, flag = _device_fan(mu, sig2, pi, None, args[0], args[1], args[2], nd, True)
    assert _same_bits(rng, e_rng) and np.isfinite(rng).all() and np.array_equal(flag, e_flag)
    assert (flag[0] == 0).all() and (flag[1] == fc.NAN_).all() and np.isnan(out[1, ..., 0]).all() and np.isfinite(out[0]).all()
    fc.check_block(out[:1], rng[:1], flag[:1], args[0], (0,), 3, nd, K, fc.judge(mu[:1], sig2[:1], pi[:1], None, (0,), True), "NaN beside")
    # a zero rounded variance: F jumps by 0.6 at 1.37
    mu3, sig23, pi3, _ = fc.make_draws(6, 1, 2, 40, 0, False)
    mu3[0, :, :], sig23[0, 0, :], sig23[0, 1, :] = np.array([[1.37], [4.0]]), 4e-6, 1.0
    pi3[0, 0, :], pi3[0, 1, :] = 0.6, 0.4
    out, rng, flag = _device_fan(mu3, sig23, pi3, None, (0.3,), (0,), 6, 40, True)
    e_out, e_rng, e_flag = fc.reference(mu3, sig23, pi3, None, (0.3,), (0,), 6, True)
    assert _same_bits(rng, e_rng) and flag[0, 0, 0] == 0 == e_flag[0, 0, 0]
    assert out[0, 0, 0, 1] <= 1.37 <= out[0, 0, 0, 2] and out[0, 0, 0, 3] < 0.3 <= out[0, 0, 0, 4] and out[0, 0, 0, 4] - out[0, 0, 0, 3] > 0.59
    raw = _device_fan(mu3, sig23, pi3, None, (0.3,), (0,), 6, 40, False)      # unrounded the variance is 4e-6: a steep, finite climb
    assert raw[2][0, 0, 0] == 0 and abs(raw[0][0, 0, 0, 0] - 1.37) < 0.01
    # weights that round to a sum of 0.99998
    mu2, sig22 = np.zeros((1, 2, 33)), np.ones((1, 2, 33))
    mu2[0, 1] = 10000.0
    pi2 = np.full((1, 2, 33), 0.499994)
    out, rng, flag = _device_fan(mu2, sig22, pi2, None, (1 - 1e-6,), (0,), 1, 33, True)
    assert flag[0, 0, 0] == fc.UNREACHED and out[0, 0, 0, 0] == rng[0, 1] == 10040.0 and abs(out[0, 0, 0, 4] - 0.99998) < 1e-14
    out, rng, flag = _device_fan(mu2, sig22, pi2, None, (1 - 1e-6, 0.5), (0,), 4, 33, True)
    assert flag[0, 0, 0] == fc.FLAT and flag[0, 0, 1] == 0 and out[0, 0, 0, 0] == out[0, 0, 0, 1] < rng[0, 1]
    raw = _device_fan(mu2, sig22, pi2, None, (1 - 1e-6,), (0,), 4, 33, False)  # unrounded the weights reach 0.999988: still short
    assert raw[2][0, 0, 0] in (fc.FLAT, fc.UNREACHED)
    # one draw: the quantile of one mixture of K normals
    mu1, sig21, pi1, A1 = fc.make_draws(9, 1, 3, 1, 3, True)
    out, rng, flag = _device_fan(mu1, sig21, pi1, A1, fc.PROBS5, (0, 2), 0, 1, True)
    assert (flag == 0).all()
    fc.check_block(out, rng, flag, fc.PROBS5, (0, 2), 0, 1, 3, fc.judge(mu1, sig21, pi1, A1, (0, 2), True, 1), "one draw")


def test_runs_entries_and_chunkings_give_the_same_bits(monkeypatch):
    """Two runs of the device entry, the host entry, and the host entry with upload chunks of one and of two slabs (R + 1 passes
    of a ring of 3 buffers over 4 and 2 chunks): the same bits in out, range and flag."""
    from hmc_jl_amd import _lib
    S = _lib.PRED_SLAB
    K, W, nd = 3, 2, 3 * S + 17
    horizons, probs, R = (0, 1, 12), fc.PROBS5, 3
    mu, sig2, pi, A = fc.make_draws(77, W, K, nd, 0, True)
    out, rng, flag = _device_fan(mu, sig2, pi, A, probs, horizons, R, nd)
    again = _device_fan(mu, sig2, pi, A, probs, horizons, R, nd)
    assert _same_bits(again[0], out) and _same_bits(again[1], rng) and np.array_equal(again[2], flag)

    def host(A_=A, hz=horizons):
        tm = _lib.Timing()
        f = _lib.predictive_quantiles(mu, sig2, pi, A_, probs, hz, R, timing=tm)
        return f, tm
    one, tm = host()
    assert tm.launches == (R + 1) * 1 + 1 + R and tm.kernel_ms > 0.0 and tm.call_ms >= tm.kernel_ms
    monkeypatch.setenv("HMCG_CHUNK_DRAWS", "1024")
    four, tm = host()
    assert tm.launches == (R + 1) * 4 + 1 + R
    monkeypatch.setenv("HMCG_CHUNK_DRAWS", "2048")
    two, tm = host()
    assert tm.launches == (R + 1) * 2 + 1 + R
    monkeypatch.delenv("HMCG_CHUNK_DRAWS")
    for f in (one, four, two):
        got = np.stack([f[name] for name in _lib.FAN_FIELDS], axis=-1)
        assert _same_bits(got, out) and _same_bits(f["range"], rng) and np.array_equal(f["flag"], flag)
    assert (flag == 0).all()
    fc.check_block(out, rng, flag, probs, horizons, R, nd, K, fc.judge(mu, sig2, pi, A, horizons, True), "entries")
    # horizon 0 alone: A is neither needed nor uploaded
    h0, _ = host(None, (0,))
    assert _same_bits(h0["quantile"][:, 0], out[:, 0, :, 0])


@pytest.mark.parametrize("K,T,nrun", [(3, 200, 700), (5, 300, 200)])
def test_device_panel_fan(K, T, nrun):
    """DevicePanel.fan on the draws `run` left in HBM (K = 5, T = 300: the sampler's own K = 5 draws -- from the LDS-resident
    kernel, there are no register-resident rows above K = 4 -- feed fan_eval_kernel<5>); the draws are unchanged afterwards."""
    from hmc_jl_amd import _lib, synth
    from hmc_jl_amd.device import DevicePanel
    W = 3
    Y, Tw, fut = synth.generate_panel(W, T, K)
    p = DevicePanel(Y, Tw, K, nrun, (12,), fut[:, 11:12])
    p.run(burnin=20, timed=False)
    horizons = (0, 12)
    f = p.fan(fc.PROBS5, horizons)                            # enqueued behind the run on the library stream
    p.sync()
    before = {n: getattr(p, n).cpu().numpy() for n in _lib.DRAW_KEYS}
    assert (p.status.cpu().numpy() == 0).all()
    timed = p.fan(fc.PROBS5, horizons, timed=True)
    assert p.last_timing.kernel_ms > 0.0 and p.last_timing.launches == 10
    out, rng, flag = (f[k].cpu().numpy() for k in ("out", "range", "flag"))
    assert _same_bits(out, timed["out"].cpu().numpy()) and (flag == 0).all()
    at = fc.judge(before["mu"], before["sig2"], before["pi_end"], before["A"], horizons, True)
    fc.check_block(out, rng, flag, fc.PROBS5, horizons, 0, nrun, K, at, "panel")
    for n in _lib.DRAW_KEYS:
        assert np.array_equal(getattr(p, n).cpu().numpy(), before[n])
    with pytest.raises(_lib.HmcgError, match="keep_draws"):
        DevicePanel(Y, Tw, K, nrun, (12,), fut[:, 11:12], keep_draws=False).fan((0.5,))


def test_estimatewindows_fan_equals_the_file_route(inflation, tmp_path):
    """code/run_hmm.jl's windows for two end dates: BatchResult.fan from the device against hmc.calcfan over the per-draw files
    saveresults writes -- each quantile inside the acceptance on the other's draws, the two within their brackets of each other
    --, and the same bits when the draws are not kept."""
    from hmc_jl_amd import hmc
    y, dates = inflation
    dd = [dt.date.fromisoformat(d) for d in dates]
    ends = [200, 201]
    horizons = (0, 12)
    kw = dict(horizons=[12], D=3, burnin=300, Nrun=1500, series="official", fan_probs=fc.PROBS5, fan_horizons=horizons)
    res = hmc.estimatewindows(y, dd, ends, keep_draws=True, **kw)
    assert (res.status == 0).all() and res.fan["quantile"].shape == (2, 2, 5) and (res.fan["flag"] == 0).all()
    for w in range(2):
        hmc.saveresults(res.samples(w), res.opts[w], str(tmp_path))
    want = [dd[e - 1] for e in ends]
    d_f, f_f = hmc.calcfan(str(tmp_path), want, fc.PROBS5, horizons)
    d_d, f_d = hmc.calcfan(str(tmp_path), want, fc.PROBS5, horizons, result=res)
    assert d_f == d_d == [str(d) for d in want] and _same_bits(f_d["quantile"], res.fan["quantile"])
    assert _same_bits(f_f["range"], f_d["range"]) and np.array_equal(f_f["flag"], f_d["flag"])
    r = res._res
    at = fc.judge(r["mu"], r["sig2"], r["pi_end"], r["A"], horizons, True)
    for f, label in ((f_d, "device"), (f_f, "files")):
        out = np.stack([f[name] for name in ("quantile", "lo", "hi", "Flo", "Fhi")], axis=-1)
        worst = fc.check_block(out, f["range"], f["flag"], fc.PROBS5, horizons, 0, 1500, 3, at, label)
        print("%s: max |F_ld(q) - p| / (B + 4 tolF) = %.3g" % (label, worst))
    gap = np.abs(f_f["quantile"] - f_d["quantile"])
    print("device vs file route: max |q - q| = %.3e" % float(gap.max()))
    assert (gap <= (f_d["hi"] - f_d["lo"]) + (f_f["hi"] - f_f["lo"])).all()
    assert (np.diff(f_d["quantile"], axis=2) > 0.0).all()
    lean = hmc.estimatewindows(y, dd, ends, keep_draws=False, **kw)
    assert _same_bits(lean.fan["quantile"], res.fan["quantile"])
    with pytest.raises(ValueError):
        lean.samples(0)
