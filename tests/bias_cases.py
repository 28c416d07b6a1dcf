"""Reference, tolerance and hand-made draws for the uncertainty-bias tests (no GPU): the np.longdouble restatement of
bias_calcs.jl's calcbias that every numeric check of hmcg_bias_moments[_device] compares against, and the bound on the
difference, derived below from the shape of the computation with no measured constant."""
import numpy as np

import predictive_cases as pc

LD = np.longdouble
U = 2.0 ** -53            # unit roundoff of fp64


def make_draws(seed, W, K, nd, pad=0, with_A=True, H=1):
    """predictive_cases.make_draws (seeded, leading dimension nd + pad, NaN in the padding) plus fcast (W, 2H, nd + pad), or
    None for H = 0.  Returns mu, pi_end, A, fcast."""
    mu, _, pi, A = pc.make_draws(seed, W, K, nd, pad, with_A)
    fc = None
    if H > 0:
        fc = np.random.default_rng(seed + 7).normal(0.3, 1.5, size=(W, 2 * H, nd + pad))
        fc[..., nd:] = np.nan
    return mu, pi, A, fc


def reference(mu, pi_end, A, fcast, horizon, round5, nd=None):
    """bias_calcs.jl:40-53 in np.longdouble on the C-ABI layouts -- mu / pi_end (W, K, ld), A (W, K, K, ld) with
    A[w, j, i, d] = A_d[i, j], fcast (W, 2H, ld) or None -- over the first nd draws; inputs through np.round(x, 5) with round5.
      futstate_d = pi_end_d A_d^horizon                       (successive row-vector x matrix products)
      covv = cov(hcat(futstate, means)), divisor nd - 1       (two-pass on v - v_0: the same number, and the reference's own
                                                               rounding then scales with the spread, not with an offset --
                                                               identical draws give exactly 0, as they must)
      nab  = mean(hcat(means, futstate))                      the OTHER column order: upstream's, kept
      uncbias = nab covv nab';  totalbias = mean(fcast[:, 1]) (NaN without fcast)
    Returns a dict of longdouble arrays: uncbias (W,), totalbias (W,), mean (W, 2K) and cov (W, 2K, 2K) in the order
    futstate | means, plus what `tolerance` needs: R (W, 2K) = max_d |v - v_0| per column and fmax (W,) = max |forecast error|."""
    rd = (lambda x: np.round(np.asarray(x, dtype=np.float64), 5)) if round5 else (lambda x: np.asarray(x, dtype=np.float64))
    nd = mu.shape[2] if nd is None else nd
    W, K, _ = mu.shape
    m = rd(mu[:, :, :nd]).astype(LD)
    w = rd(pi_end[:, :, :nd]).astype(LD)
    if horizon > 0:
        At = rd(A[:, :, :, :nd]).astype(LD)
    for _ in range(horizon):
        nw = np.empty_like(w)
        for c in range(K):
            t = w[:, 0] * At[:, c, 0]
            for i in range(1, K):
                t = t + w[:, i] * At[:, c, i]
            nw[:, c] = t
        w = nw
    v = np.concatenate([w, m], axis=1)                                   # (W, 2K, nd): futstate | means
    n = LD(nd)
    with np.errstate(invalid="ignore", divide="ignore"):
        x = v - v[:, :, :1]
        mx = x.sum(axis=2) / n
        mean = v[:, :, 0] + mx
        dv = x - mx[:, :, None]
        cov = np.einsum("wad,wbd->wab", dv, dv) / (n - LD(1))
        nab = np.concatenate([mean[:, K:], mean[:, :K]], axis=1)         # means | futstate
        unc = np.einsum("wa,wab,wb->w", nab, cov, nab)
        R = np.nanmax(np.abs(x), axis=2)
        if fcast is None:
            tot = np.full(W, np.nan, dtype=LD)
            fmax = np.zeros(W, dtype=LD)
        else:
            fe = rd(fcast[:, 1, :nd]).astype(LD)
            tot = fe.sum(axis=1) / n
            fmax = np.nanmax(np.abs(fe), axis=1)
    return {"uncbias": unc, "totalbias": tot, "mean": mean, "cov": cov, "R": R, "fmax": fmax}


def tolerance(ref, nd, K, horizon):
    """Absolute bounds on |fp64 result - reference| per output cell, for an fp64 computation of the library's shape: moments of
    x_a = v_a - p_a about the pivot p = v of draw 0, n = nd terms summed in SOME fixed order, one FMA per product.  u = 2^-53,
    R_a = max_d |v_a - p_a| (taken from the reference), first order in u.  Nothing here is measured.

    Inputs.  mu columns are exact.  An omega entry comes from h = horizon products with a row-stochastic matrix: each dot product
    of K terms (|omega| <= 1) errs by at most K u, a stochastic matrix does not amplify what is there, so after h steps at
    most K h u; the 5-digit rounding lets rows sum to 1 +- K 5e-6, covered by doubling: eps = 2 K h u per omega entry, 0 for a mu
    column.  v and the pivot both carry it: e_a = 2 eps_a on x_a, plus u R_a for the subtraction.

    cov.  Each product x_a x_b inherits R_b (e_a + u R_a) + R_a (e_b + u R_b); n of them: n (R_a e_b + R_b e_a) + 2 n u R_a R_b.
    Summing n terms bounded by R_a R_b in any order: (n - 1) u n R_a R_b.  S1_a likewise: n (n u R_a + e_a), so S1_a S1_b / n
    (|S1| <= n R) errs by 2 n^2 u R_a R_b + n (R_a e_b + R_b e_a) + 2 u n R_a R_b; the subtraction and the division by n - 1 add
    2 u |numerator| <= 4 u n R_a R_b.  Numerator: (3 n^2 + 7 n) u R_a R_b + 2 n (R_a e_b + R_b e_a); over n - 1 >= n / 2:
        tol_cov[a, b] = (3 n + 7) 2^-52 R_a R_b + 4 (R_a e_b + R_b e_a),      e_a = 4 K h u (omega columns), 0 (mu columns).
    The longdouble reference's own error has the same shape with 2^-64 for u (|dv| <= 2 R, each carrying (n + 1) 2^-64 R from the
    mean): 16 (n + 1) 2^-64 R_a R_b, added; it vanishes with R.
    mean_a = p_a + S1_a / n: eps_a (pivot) + (n u R_a + e_a) + u R_a (division) + u |mean_a| (last addition):
        tol_mean[a] = (n + 1) u R_a + 3 eps_a + u |mean_a|.
    uncbias = sum_ab nab_a cov_ab nab_b inherits sum |nab_a| |nab_b| tol_cov[a, b], the mean errors through
    sum (tol_nab_a |cov_ab| |nab_b| + |nab_a| |cov_ab| tol_nab_b), and (4 K + 2) u sum |nab_a cov_ab nab_b| for its own 2K-term
    dot products.
    totalbias: the pivoted sum of n terms bounded by 2 max |x|, divided by n: n 2^-52 max |x|.

    Returns a dict of float64 arrays shaped like the outputs: cov (W, 2K, 2K), mean (W, 2K), uncbias (W,), totalbias (W,).  NaN
    reference cells give NaN bounds; those cells are compared by position only."""
    n = float(nd)
    R = ref["R"].astype(np.float64)
    mean = ref["mean"].astype(np.float64)
    cov = ref["cov"].astype(np.float64)
    eps = np.zeros(2 * K)
    eps[:K] = 2.0 * K * horizon * U
    e = 2.0 * eps
    with np.errstate(invalid="ignore"):
        tol_cov = ((3.0 * n + 7.0) * 2.0 * U + 16.0 * (n + 1.0) * 2.0 ** -64) * R[:, :, None] * R[:, None, :] + 4.0 * (R[:, :, None] * e[None, None, :] + R[:, None, :] * e[None, :, None])
        tol_mean = (n + 1.0) * U * R + 3.0 * eps[None, :] + U * np.abs(mean)
        nab = np.abs(np.concatenate([mean[:, K:], mean[:, :K]], axis=1))
        tnab = np.concatenate([tol_mean[:, K:], tol_mean[:, :K]], axis=1)
        acov = np.abs(cov)
        tol_unc = (np.einsum("wa,wab,wb->w", nab, tol_cov, nab) + 2.0 * np.einsum("wa,wab,wb->w", tnab, acov, nab)
                   + (4.0 * K + 2.0) * U * np.einsum("wa,wab,wb->w", nab, acov, nab))
        tol_tot = n * 2.0 * U * ref["fmax"].astype(np.float64)
    return {"cov": tol_cov, "mean": tol_mean, "uncbias": tol_unc, "totalbias": tol_tot}


def check(got, ref, tol, label=""):
    """got: dict of float64 arrays (uncbias / uncerbias, totalbias, mean, cov).  NaN positions must match the reference's exactly;
    finite cells lie within tol.  Prints and returns the largest difference in units of its bound."""
    worst = 0.0
    for key in ("uncbias", "totalbias", "mean", "cov"):
        g = np.asarray(got["uncerbias" if key == "uncbias" and "uncerbias" in got else key], dtype=np.float64)
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
        print("%s %-9s max |diff| = %.3e, bound there %.3e, worst diff/bound = %.3g" % (label, key, float(diff.max()), float(bound[np.argmax(diff)]), ratio))
        assert (diff <= bound).all(), (label, key, float(diff.max()), ratio)
        worst = max(worst, ratio)
    return worst
