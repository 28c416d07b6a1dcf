"""Reference and tolerance for the predictive-mixture moment tests (no GPU): the np.longdouble restatement of the table in
include/hmcg.h that every numeric check of hmcg_mixture_moments[_device] compares against, and the bound on the difference,
derived below from the shape of the computation with no measured constant.  The draws come from predictive_cases.make_draws
(seeded, C-ABI layouts, NaN in the padding)."""
import numpy as np

import predictive_cases as pc

LD = np.longdouble
U = 2.0 ** -53            # unit roundoff of fp64
FIELDS = ("mean", "variance", "skewness", "kurtosis", "within", "between", "draw_skewness", "weight")

make_draws = pc.make_draws


def omegas(pi_end, A, horizon, dtype=LD):
    """pi_end A^horizon per draw, (W, K, nd): successive row-vector x matrix products on A[w, j, i, d] = A_d[i, j]."""
    w = pi_end.astype(dtype)
    K = w.shape[1]
    if horizon > 0:
        At = A.astype(dtype)
    for _ in range(horizon):
        nw = np.empty_like(w)
        for c in range(K):
            t = w[:, 0] * At[:, c, 0]
            for i in range(1, K):
                t = t + w[:, i] * At[:, c, i]
            nw[:, c] = t
        w = nw
    return w


def reference(mu, sig2, pi_end, A, horizons, round5, nd=None):
    """The eight outputs per (window, horizon) in np.longdouble on the C-ABI layouts -- mu / sig2 / pi_end (W, K, ld),
    A (W, K, K, ld) with A[w, j, i, d] = A_d[i, j] -- over the first nd draws; inputs through np.round(x, 5) with round5.
    Two-pass and central: the pooled mean M first (as x0 + sum omega (mu - x0) / sum omega with x0 = mu of state 0 of draw 0, a
    shift of the data that keeps the reference's own rounding at the scale of the spread), then the central moments
    sum omega g_i(mu - M, v) / sum omega with g_2 = D^2 + v, g_3 = D (D^2 + 3 v), g_4 = D^4 + 6 D^2 v + 3 v^2; per draw the
    mean, variance and skewness of its own normalised mixture.  It shares neither the pivot c nor the raw-moment polynomials
    with the library.
    Returns a dict of (W, n_h) longdouble arrays under FIELDS, plus what `tolerance` needs, each (W, n_h): R = max |mu - c| over
    draws and states with c the mixture mean of draw 0, V = max sig2, smin / smax = min / max over the draws of sum_k omega_k,
    vdmin = the smallest per-draw variance, skmax = the largest |per-draw skewness|, mumax = max |mu|."""
    rd = (lambda x: np.round(np.asarray(x, dtype=np.float64), 5)) if round5 else (lambda x: np.asarray(x, dtype=np.float64))
    nd = mu.shape[2] if nd is None else nd
    W, K, _ = mu.shape
    m = rd(mu[:, :, :nd]).astype(LD)
    v = rd(sig2[:, :, :nd]).astype(LD)
    pe = rd(pi_end[:, :, :nd])
    At = rd(A[:, :, :, :nd]) if any(h > 0 for h in horizons) else None
    out = {k: np.empty((W, len(horizons)), dtype=LD) for k in FIELDS + ("R", "V", "smin", "smax", "vdmin", "skmax", "mumax")}
    n = LD(nd)
    for j, h in enumerate(horizons):
        w = omegas(pe, At, h)
        with np.errstate(invalid="ignore", divide="ignore"):
            s = w.sum(axis=1)                                            # (W, nd)
            P0 = s.sum(axis=1)
            x0 = m[:, 0, 0]
            M = x0 + (w * (m - x0[:, None, None])).sum(axis=(1, 2)) / P0
            D = m - M[:, None, None]
            D2 = D * D
            var = (w * (D2 + v)).sum(axis=(1, 2)) / P0
            c3 = (w * D * (D2 + 3 * v)).sum(axis=(1, 2)) / P0
            c4 = (w * (D2 * D2 + 6 * D2 * v + 3 * v * v)).sum(axis=(1, 2)) / P0
            md = x0[:, None] + (w * (m - x0[:, None, None])).sum(axis=1) / s       # per-draw mean (W, nd)
            e = m - md[:, None, :]
            vd = (w * (e * e + v)).sum(axis=1) / s
            skd = (w * e * (e * e + 3 * v)).sum(axis=1) / s / (vd * np.sqrt(vd))
            mbar = x0 + (md - x0[:, None]).sum(axis=1) / n
            out["mean"][:, j] = M
            out["variance"][:, j] = var
            out["skewness"][:, j] = c3 / (var * np.sqrt(var))
            out["kurtosis"][:, j] = c4 / (var * var) - 3
            out["within"][:, j] = vd.sum(axis=1) / n
            out["between"][:, j] = ((md - mbar[:, None]) ** 2).sum(axis=1) / n
            out["draw_skewness"][:, j] = skd.sum(axis=1) / n
            out["weight"][:, j] = P0 / n
            out["R"][:, j] = np.abs(m - md[:, None, :1]).max(axis=(1, 2))
            out["V"][:, j] = np.abs(v).max(axis=(1, 2))
            out["smin"][:, j], out["smax"][:, j] = s.min(axis=1), s.max(axis=1)
            out["vdmin"][:, j], out["skmax"][:, j] = vd.min(axis=1), np.abs(skd).max(axis=1)
            out["mumax"][:, j] = np.abs(m).max(axis=(1, 2))
    return out


def tolerance(ref, nd, K, horizons):
    """Absolute bounds on |fp64 result - reference| per output cell, for an fp64 computation of the library's shape: per draw
    the closed-form terms about a pivot c near the mixture mean of draw 0, n = nd draws summed in SOME fixed order, first order
    in u = 2^-53.  Every magnitude below is taken from the reference; nothing is measured on the code under test.

    Magnitudes.  R = max |mu - c| (+ (K + 2) u max |mu|: the library's c is the fp64 value of draw 0's mean), V = max sig2,
    s_d = sum_k omega_k in [sm, Om] (1 up to the 5-digit rounding of the rows).  Term bounds of the four polynomials:
    T1 = R, T2 = R^2 + V, T3 = R (R^2 + 3 V), T4 = R^4 + 6 R^2 V + 3 V^2.  The algebra is exact for ANY c, so the error of c
    itself costs nothing.

    Weights.  An omega entry comes from h products with a row-stochastic matrix: each dot product of K terms errs by at most
    K u Om, a stochastic matrix does not amplify what is there; doubled as in bias_cases: ew = 2 K h u Om per weight.

    Pooled sums.  delta = fl(mu - c) carries u R.  g_i(delta, v) evaluated in floating point errs by at most c_i u T_i with
    c_i <= 10 roundings (i for the powers of delta, the rest for the operations).  A draw's term sum_k omega g_i (K FMAs):
    (K ew + (10 + K) u Om) T_i.  n such terms, each at most Om T_i, added in any order: (n - 1) u n Om T_i.  So
        |err P_i| <= n Om T_i eta,   eta = K ew / Om + (10 + K + n) u,
    and the same eta covers P0 = sum s_d.  m_i = P_i / P0 with P0 >= n sm and |m_i| <= T_i:
        |err m_i| <= theta T_i,      theta = 2 (Om / sm) eta + u.
    mean = c + m1:                               theta R + u |mean|.
    variance = m2 - m1^2:                        E_var = (theta + u) (T2 + 2 R^2).
    skewness = N3 / var^1.5, N3 = m3 - 3 m1 m2 + 2 m1^3, |terms| <= B3 = T3 + 3 R T2 + 2 R^3; the m_i errors give
      theta (T3 + 6 R T2 + 6 R^3) <= 3 theta B3, the six operations 6 u B3; the denominator 1.5 E_var / var + 2 u relative,
      three more roundings:                      (3 theta + 6 u) B3 / var^1.5 + |skew| (1.5 E_var / var + 5 u).
    kurtosis = N4 / var^2 - 3, B4 = T4 + 4 R T3 + 6 R^2 T2 + 3 R^4, errors theta (T4 + 8 R T3 + 18 R^2 T2 + 12 R^4) <= 4 theta B4:
                                                 (4 theta + 8 u) B4 / var^2 + |kurt + 3| (2 E_var / var + 4 u) + u (|kurt| + 3).
    Per-draw quantities.  a = (sum omega delta) (1 / s): |err a| <= al R, al = 2 (K ew + (K + 1) u Om) / sm + 2 u; e = delta - a,
    |e| <= 2 R, err (al + 3 u) R.  Terms omega (e^2 + v) <= T2e = 4 R^2 + V, omega e (e^2 + 3 v) <= T3e = 2 R (4 R^2 + 3 V):
      E_vd  = [2 K ew T2e + Om (4 (al + 3 u) R^2 + (4 + 2 K) u T2e)] / sm + 2 u T2e                        per-draw variance
      E_m3d = [2 K ew T3e + Om ((al + 3 u) R (12 R^2 + 3 V) + (6 + 2 K) u T3e)] / sm + 2 u T3e              per-draw third moment
    within = sum var_d / n:                      E_vd + (n + 1) u T2e.
    draw_skewness = sum skew_d / n:              E_m3d / vdmin^1.5 + skmax (1.5 E_vd / vdmin + 5 u) + (n + 1) u skmax.
    between = Q2 / n - (Q1 / n)^2, b = a_d - a_0, |b| <= 2 R, E_b = 2 al R + 2 u R; E_q1 = E_b + (n + 1) u 2 R;
      E_q2 = 4 R E_b + (n + 3) u 4 R^2:          E_q2 + 4 R E_q1 + 12 u R^2.
    weight = P0 / n:                             K ew + (K + n + 1) u Om.
    The longdouble reference has the same shape with 2^-64 for u and terms at most 2^4 larger (|mu - M| <= 2 R): every bound is
    multiplied by 1 + 2^-6.

    Returns a dict of float64 (W, n_h) arrays under FIELDS.  NaN reference cells give NaN bounds; those cells are compared by
    position only."""
    n = float(nd)
    f = lambda k: ref[k].astype(np.float64)
    V, sm, Om = f("V"), f("smin"), f("smax")
    h = np.asarray(horizons, dtype=np.float64)[None, :]
    u = U
    with np.errstate(invalid="ignore", divide="ignore"):
        R = f("R") + (K + 2) * u * f("mumax")
        ew = 2.0 * K * h * u * Om
        T1, T2, T3, T4 = R, R * R + V, R * (R * R + 3 * V), R ** 4 + 6 * R * R * V + 3 * V * V
        eta = K * ew / Om + (10 + K + n) * u
        theta = 2 * (Om / sm) * eta + u
        mean, var, sk, ku = f("mean"), f("variance"), f("skewness"), f("kurtosis")
        E_var = (theta + u) * (T2 + 2 * R * R)
        B3 = T3 + 3 * R * T2 + 2 * R ** 3
        B4 = T4 + 4 * R * T3 + 6 * R * R * T2 + 3 * R ** 4
        al = 2 * (K * ew + (K + 1) * u * Om) / sm + 2 * u
        T2e, T3e = 4 * R * R + V, 2 * R * (4 * R * R + 3 * V)
        E_vd = (2 * K * ew * T2e + Om * (4 * (al + 3 * u) * R * R + (4 + 2 * K) * u * T2e)) / sm + 2 * u * T2e
        E_m3d = (2 * K * ew * T3e + Om * ((al + 3 * u) * R * (12 * R * R + 3 * V) + (6 + 2 * K) * u * T3e)) / sm + 2 * u * T3e
        vdmin, skmax = f("vdmin"), f("skmax")
        E_b = 2 * al * R + 2 * u * R
        E_q1 = E_b + (n + 1) * u * 2 * R
        E_q2 = 4 * R * E_b + (n + 3) * u * 4 * R * R
        tol = {
            "mean": theta * T1 + u * np.abs(mean),
            "variance": E_var,
            "skewness": (3 * theta + 6 * u) * B3 / var ** 1.5 + np.abs(sk) * (1.5 * E_var / var + 5 * u),
            "kurtosis": (4 * theta + 8 * u) * B4 / (var * var) + np.abs(ku + 3) * (2 * E_var / var + 4 * u) + u * (np.abs(ku) + 3),
            "within": E_vd + (n + 1) * u * T2e,
            "between": E_q2 + 4 * R * E_q1 + 12 * u * R * R,
            "draw_skewness": E_m3d / vdmin ** 1.5 + skmax * (1.5 * E_vd / vdmin + 5 * u) + (n + 1) * u * skmax,
            "weight": K * ew + (K + n + 1) * u * Om,
        }
    return {k: t * (1.0 + 2.0 ** -6) for k, t in tol.items()}


def check(got, ref, tol, label="", fields=FIELDS):
    """got: dict of float64 (W, n_h) arrays under FIELDS.  NaN positions must match the reference's exactly; finite cells lie
    within tol.  Prints the largest difference per field in units of its bound and returns {field: worst diff / bound}."""
    worst = {}
    for key in fields:
        g = np.asarray(got[key], dtype=np.float64)
        r = ref[key]
        assert g.shape == r.shape, (key, g.shape, r.shape)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (label, key, "NaN positions differ", g, r)
        ok = ~np.isnan(r)
        if not ok.any():
            continue
        diff = np.abs(g.astype(LD) - r)[ok].astype(np.float64)
        bound = np.broadcast_to(tol[key], r.shape)[ok]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = float(np.max(np.where(diff == 0.0, 0.0, diff / bound)))         # a difference under a zero bound: inf
        print("%s %-13s max |diff| = %.3e, bound there %.3e, worst diff/bound = %.3g" % (label, key, float(diff.max()), float(bound[np.argmax(diff)]), ratio))
        assert (diff <= bound).all(), (label, key, float(diff.max()), ratio)
        worst[key] = ratio
    return worst
