"""Reference, tolerance and cases for the autocorrelation tests (no GPU): numpy restatements of the rules of
hmcg_chain_autocorr[_device] in include/hmcg.h that every check compares against.

`reference`: a_d = x'_d - p is the fp64 subtraction the ABI defines (p = x' of draw 0); from there every sum -- S1, S2, the
lagged sums C_l, the edge sums H_l and T_l, the half sums of the split-R-hat -- and acov, mean, variance and rhat are taken in
np.longdouble.  `derived` is the fp64 restatement of the ABI's derived block (rho, Geyer's initial monotone sequence, ess,
mcse), operation for operation; `device_sums` restates the library's six running sums (the thirds [0, h), [h, n - h),
[n - h, n) per 1024-draw slab: thread t of 256 takes the slab's draws t, t + 256, .. in order with unfused squares, an xor
butterfly over the 64 lanes, the four waves in order, the slabs in order) and `rhat_of_sums` the split-R-hat from them, so that
every derived output can be compared bit for bit with what the device made of its own acov and sums.

Tolerance of acov_l, derived from the shape of the library's computation, nothing measured.  u = 2^-53, n draws, a exact in
both computations.  Write A_l = sum |a_d a_(d-l)|, M = sum |a_d| / n >= |m|, Q_l = 2 sum |a_d| + sum_{d < l} |a_d| +
sum_{d >= n-l} |a_d| >= |2 S1 - H_l - T_l|.
  C_l: n - l products, each fused into its addition (one rounding), merged by additions in some fixed tree (additions of an
    exact zero -- the padding of a slab, an idle share -- are exact): at most n - l inexact operations on any path, error at
    most n u A_l.
  S1: at most n - 1 inexact additions, error (n - 1) u sum |a|; H_l and T_l: l - 1 additions each over their l terms.  So
    q = 2 S1 - H_l - T_l errs by at most (n - 1) u Q_l from its terms (l <= n - 1) plus 2 u Q_l from its two subtractions:
    (n + 1) u Q_l.  m = S1 / n errs by at most ((n - 1) u sum |a| + u |S1|) / n <= n u M.
  m q: |dm| Q_l + M |dq| + u M Q_l <= (2 n + 2) u M Q_l.
  (n - l) m m, n - l exact: two factors m with error n u M each and two roundings: (2 n + 2) u (n - l) M^2.
  r = C_l - m q, r + s and the division by n: three roundings of at most A_l + M Q_l + (n - l) M^2 each.
  Sum, over n: [(n + 3) A_l + (2 n + 5) M Q_l + (2 n + 5) (n - l) M^2] u / n; three more u for the second-order terms and the
  longdouble reference's own rounding (2^-64 in place of u).
  Bound: (2 n + 8) u (A_l + M Q_l + (n - l) M^2) / n.  A constant column has a = 0: the bound is 0 and the library gives exactly 0.
Mean and variance: the bounds of density_cases (same formulas, any fixed summation order): (n + 3) u R + u |mean| and
(3 n + 7) 2^-52 R^2, R = max |a_d|.
Cells where the reference is NaN must be NaN (a non-finite value anywhere in a column makes every acov of it NaN in the
reference as in the library)."""
import numpy as np

from density_cases import LD, SLAB, U, round5

FIELDS = ("mean", "variance", "tau", "ess", "mcse", "pairs", "truncated", "rhat")
NT, LANES = 256, 64
LAG_EDGES = (0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 255, 256, 1023, 1024)      # 8 lags a thread; the thread split changes at 16, 32, ..


def prepare(x, round5_=True, nd=None):
    """x (W, ..., ld) -> x' (W, C, nd), p (W, C, 1) and a = x' - p in fp64."""
    x = np.asarray(x, dtype=np.float64)
    W, ld = x.shape[0], x.shape[-1]
    nd = ld if nd is None else int(nd)
    xs = x.reshape(W, -1, ld)[:, :, :nd]
    xr = round5(xs) if round5_ else xs.copy()
    p = xr[:, :, :1].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        a = xr - p
    return xr, p, a


def geyer(acov, variance, n):
    """The derived block for one column in fp64, operation for operation: (tau, ess, mcse, pairs, truncated, [P_k used or
    stopping])."""
    nan = np.float64(np.nan)
    a0 = np.float64(acov[0])
    n = np.float64(n)
    if not (a0 > 0.0):
        return nan, nan, nan, 0, 0, []
    npairs = len(acov) // 2
    tau, prev = np.float64(-1.0), np.float64(np.inf)
    k, Ps = 0, []
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        while k < npairs:
            ra = np.float64(acov[2 * k]) / a0
            rb = np.float64(acov[2 * k + 1]) / a0
            P = ra + rb
            Ps.append(float(P))
            if not (P > 0.0):
                break
            if P > prev:
                P = prev
            tau = tau + np.float64(2.0) * P
            prev = P
            k += 1
        truncated = 1 if k == npairs else 0
        if k == 0:
            tau = nan
        ess = n / tau
        mcse = np.sqrt((np.float64(variance) * tau) / n)
    return tau, ess, mcse, k, truncated, Ps


def derived(acov, variance, n):
    """geyer over (W, C, L + 1) acov and (W, C) variance: a dict of (W, C) arrays tau, ess, mcse, pairs, truncated."""
    acov = np.asarray(acov, dtype=np.float64)
    W, Cn = acov.shape[:2]
    out = {k: np.empty((W, Cn)) for k in ("tau", "ess", "mcse")}
    out["pairs"] = np.zeros((W, Cn), dtype=np.int64)
    out["truncated"] = np.zeros((W, Cn), dtype=bool)
    out["P"] = [[None] * Cn for _ in range(W)]
    for w in range(W):
        for c in range(Cn):
            tau, ess, mcse, k, tr, Ps = geyer(acov[w, c], variance[w, c], n)
            out["tau"][w, c], out["ess"][w, c], out["mcse"][w, c] = tau, ess, mcse
            out["pairs"][w, c], out["truncated"][w, c] = k, bool(tr)
            out["P"][w][c] = Ps
    return out


def device_sums(a):
    """The library's six running sums (S1, S2 of [0, h), [h, n - h), [n - h, n)) of a (W, C, n) in fp64, in its own order."""
    W, Cn, n = a.shape
    h = n // 2
    nslab = (n + SLAB - 1) // SLAB
    pad = np.zeros((W, Cn, nslab * SLAB))
    pad[:, :, :n] = a
    d = np.arange(nslab * SLAB)
    third = np.where(d < h, 0, np.where(d < n - h, 1, 2))
    rs = np.zeros((W, Cn, 6))
    lane = np.arange(LANES)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(nslab):
            blk = pad[:, :, s * SLAB:(s + 1) * SLAB]
            th = third[s * SLAB:(s + 1) * SLAB]
            for q in range(3):
                u = np.where(th == q, blk, 0.0).reshape(W, Cn, SLAB // NT, NT)      # [k][tid]: draw tid + 256 k of the slab
                s1 = np.zeros((W, Cn, NT))
                s2 = np.zeros((W, Cn, NT))
                for k in range(SLAB // NT):
                    sq = u[:, :, k] * u[:, :, k]
                    s1 = s1 + u[:, :, k]
                    s2 = s2 + sq
                for e, v in ((2 * q, s1), (2 * q + 1, s2)):
                    v = v.reshape(W, Cn, NT // LANES, LANES)
                    for m in (32, 16, 8, 4, 2, 1):
                        v = v + v[..., lane ^ m]
                    t = v[..., 0, 0]
                    for wv in range(1, NT // LANES):
                        t = t + v[..., wv, 0]
                    rs[:, :, e] = rs[:, :, e] + t
    return rs


def moments_of_sums(rs, p, n):
    """mean, variance and rhat from the six sums, every operation a rounded fp64 operation of its own (include/hmcg.h)."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        n_ = np.float64(n)
        S1 = (rs[..., 0] + rs[..., 2]) + rs[..., 4]
        S2 = (rs[..., 1] + rs[..., 3]) + rs[..., 5]
        m = S1 / n_
        mean = p[..., 0] + m
        variance = (S2 - (S1 * S1) / n_) / (n_ - np.float64(1.0))
        hh = np.float64(n // 2)
        hm1 = hh - np.float64(1.0)
        m1, m2 = rs[..., 0] / hh, rs[..., 4] / hh
        v1 = (rs[..., 1] - (rs[..., 0] * rs[..., 0]) / hh) / hm1
        v2 = (rs[..., 5] - (rs[..., 4] * rs[..., 4]) / hh) / hm1
        Wv = (v1 + v2) / np.float64(2.0)
        dm = m1 - m2
        varplus = ((hm1 / hh) * Wv + (dm * dm) / np.float64(2.0)) + (rs[..., 2] - rs[..., 2])
        rhat = np.sqrt(varplus / Wv)
    return mean, variance, rhat


def reference(x, L, round5_=True, nd=None):
    """The long-double reference: acov (W, C, L + 1), mean, variance, rhat (W, C) as longdouble; tau, ess, mcse, pairs,
    truncated and the pair sums P from `derived` applied to its own acov and variance rounded to fp64; and the magnitudes
    `tolerance` needs."""
    xr, p, a = prepare(x, round5_, nd)
    W, Cn, n = a.shape
    L = int(L)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        aL = a.astype(LD)
        nL = LD(n)
        S1 = aL.sum(axis=2)
        S2 = (aL * aL).sum(axis=2)
        m = S1 / nL
        mean = p[..., 0].astype(LD) + m
        variance = (S2 - S1 * S1 / nL) / (nL - 1)
        absa = np.abs(a)
        A1 = absa.sum(axis=2)
        M = A1 / n
        acov = np.empty((W, Cn, L + 1), dtype=LD)
        bound = np.empty((W, Cn, L + 1))
        H = np.zeros((W, Cn), dtype=LD)
        T = np.zeros((W, Cn), dtype=LD)
        Ha = np.zeros((W, Cn))
        Ta = np.zeros((W, Cn))
        for l in range(L + 1):
            if l > 0:
                H = H + aL[:, :, l - 1]
                T = T + aL[:, :, n - l]
                Ha = Ha + absa[:, :, l - 1]
                Ta = Ta + absa[:, :, n - l]
            Cl = (aL[:, :, l:] * aL[:, :, :n - l]).sum(axis=2)
            Al = (absa[:, :, l:] * absa[:, :, :n - l]).sum(axis=2)
            acov[:, :, l] = (Cl - m * (2 * S1 - H - T) + (n - l) * m * m) / nL
            bound[:, :, l] = (2.0 * n + 8.0) * U * (Al + M * (2.0 * A1 + Ha + Ta) + (n - l) * M * M) / n
        h = n // 2
        hL = LD(h)
        first, second = aL[:, :, :h], aL[:, :, n - h:]
        m1, m2 = first.sum(axis=2) / hL, second.sum(axis=2) / hL
        v1 = ((first * first).sum(axis=2) - first.sum(axis=2) ** 2 / hL) / (hL - 1)
        v2 = ((second * second).sum(axis=2) - second.sum(axis=2) ** 2 / hL) / (hL - 1)
        Wv = (v1 + v2) / 2
        mid = aL[:, :, h:n - h].sum(axis=2)
        rhat = np.sqrt((((hL - 1) / hL * Wv + (m1 - m2) ** 2 / 2) + (mid - mid)) / Wv)
        R = absa.max(axis=2)
    out = {"acov": acov, "mean": mean, "variance": variance, "rhat": rhat, "acov_bound": bound, "R": R, "n": n, "L": L}
    out.update(derived(acov.astype(np.float64), variance.astype(np.float64), n))
    return out


def tolerance(ref):
    """Absolute bounds per cell of acov, mean and variance (module docstring)."""
    n = float(ref["n"])
    R = ref["R"]
    with np.errstate(invalid="ignore", over="ignore"):
        return {"acov": ref["acov_bound"], "mean": (n + 3.0) * U * R + U * np.abs(ref["mean"].astype(np.float64)),
                "variance": (3.0 * n + 7.0) * 2.0 * U * R * R}


def restate(got, x, round5_=True, nd=None):
    """What the ABI's derived block makes of the device's own acov, variance and sums: the dict of FIELDS (fp64)."""
    _, p, a = prepare(x, round5_, nd)
    n = a.shape[2]
    mean, variance, rhat = moments_of_sums(device_sums(a), p, n)
    out = derived(got["acov"], got["variance"], n)
    out.update({"mean": mean, "variance": variance, "rhat": rhat})
    return out


def check(got, ref, x, round5_=True, nd=None, label=""):
    """got: the dict of _lib.unpack_chain_autocorr.  (a) acov, mean and variance within `tolerance`, NaN positions exactly;
    (b) tau, ess, mcse, pairs, truncated and rhat array_equal (NaN positions included) with `restate` -- and mean and variance
    too, which the restated sums give bit for bit.  Prints and returns the largest |diff| / bound per output of (a)."""
    tol = tolerance(ref)
    worst = {}
    for key in ("acov", "mean", "variance"):
        g, r = np.asarray(got[key], dtype=np.float64), ref[key]
        assert g.shape == r.shape, (label, key, g.shape, r.shape)
        rf = r.astype(np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(rf)), (label, key, "NaN positions differ")
        inf = np.isinf(rf)
        assert np.array_equal(g[inf], rf[inf]), (label, key, "infinities differ")
        ok = np.isfinite(rf)
        if not ok.any():
            worst[key] = 0.0
            continue
        assert np.isfinite(g[ok]).all(), (label, key, "non-finite where the reference is finite")
        diff = np.abs(g[ok].astype(LD) - r[ok]).astype(np.float64)
        bound = tol[key][ok]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = float(np.max(np.where(diff == 0.0, 0.0, diff / bound)))
        print("%s %-8s max |diff| = %.3e, bound there %.3e, worst diff/bound = %.3g" % (label, key, float(diff.max()), float(bound[np.argmax(diff)]), ratio))
        assert (diff <= bound).all(), (label, key, float(diff.max()), ratio)
        worst[key] = ratio
    want = restate(got, x, round5_, nd)
    for key in FIELDS:
        g, r = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == r.shape and g.dtype == r.dtype, (label, key, g.shape, r.shape, g.dtype, r.dtype)
        assert np.array_equal(g, r, equal_nan=g.dtype == np.float64), (label, key, g, r)
    return worst


def ar1(seed, phi, n, offset=0.0, scale=1.0):
    """A stationary AR(1) chain x_t = phi x_(t-1) + e_t of length n (unit innovations), times scale, plus offset."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(n)
    x = np.empty(n)
    x[0] = e[0] / np.sqrt(1.0 - phi * phi)
    for t in range(1, n):
        x[t] = phi * x[t - 1] + e[t]
    return offset + scale * x


def make_case(seed, W, Cn, nd, pad=0):
    """(W, Cn, nd + pad) draws, NaN in the padding (finite outputs then prove it unread).  Column c plays the part c % 4:
    0 an AR(1) chain with phi = 0.7; 1 white noise offset by 1e4 with a spread of 1e-2; 2 an AR(1) chain with phi = -0.5;
    3 a slowly mixing chain (phi = 0.98) about 3."""
    rng = np.random.default_rng(seed)
    x = np.full((W, Cn, nd + pad), np.nan)
    for w in range(W):
        for c in range(Cn):
            s = int(rng.integers(1 << 30))
            part = c % 4
            if part == 0:
                v = ar1(s, 0.7, nd)
            elif part == 1:
                v = 1e4 + 1e-2 * np.random.default_rng(s).standard_normal(nd)
            elif part == 2:
                v = ar1(s, -0.5, nd, 1.5, 0.3)
            else:
                v = ar1(s, 0.98, nd, 3.0, 0.1)
            x[w, c, :nd] = v
    return x


AR1_PHIS = (0.0, 0.5, 0.9, -0.5, 0.5)      # the last chain is offset by 1e4
AR1_N, AR1_LAGS = 50000, 199
_AR1 = []


def ar1_suite():
    """The seeded AR(1) chains (1, 5, AR1_N) of the tests and their reference with AR1_LAGS lags, no rounding; computed once."""
    if not _AR1:
        x = np.stack([ar1(100 + i, phi, AR1_N, 1e4 if i == 4 else 0.0) for i, phi in enumerate(AR1_PHIS)])[None]
        x.setflags(write=False)
        _AR1.append((x, reference(x, AR1_LAGS, False)))
    return _AR1[0]
