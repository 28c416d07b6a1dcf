"""Reference and hand-made draws for the predictive-CDF tests (no GPU): the float64 numpy recomputation every numeric check
of hmcg_predictive_cdf[_device] compares against, and the seeded generator of draw arrays in the C-ABI layouts."""
import math

import numpy as np

_erfc = np.frompyfunc(math.erfc, 1, 1)


def tolerance(nd, K, h_max):
    """Absolute bound on |device - reference|, derived: every term lies in [0, 1]; the summation order moves a mean that is at
    most 1 by at most nd 2^-53; erfc to a few ulps and the hoisted 1 / (sqrt 2 sqrt(var)) (|z phi(z)| <= 0.242 times a few ulps
    of z) stay under 32 2^-52 per draw, and per-draw errors are averaged; FMA contraction in the omega recurrence K h 2^-53."""
    return (nd + 64 + 2 * K * h_max) * 2.0 ** -52


def reference(mu, sig2, pi_end, A, grid, horizons, round5, nd=None):
    """cdf (W, n_h, G) from draw arrays in the C-ABI layouts -- mu/sig2/pi_end (W, K, ld), A (W, K, K, ld) with
    A[w, j, i, d] = A_d[i, j] -- over their first nd draws: inputs through np.round(x, 5) with round5, omega by successive
    vector-matrix products (k ascending), Phi via math.erfc, the mean by np.mean."""
    rd = (lambda x: np.round(np.asarray(x, dtype=np.float64), 5)) if round5 else (lambda x: np.asarray(x, dtype=np.float64))
    nd = mu.shape[2] if nd is None else nd
    mu, sig2, pi = rd(mu[:, :, :nd]), rd(sig2[:, :, :nd]), rd(pi_end[:, :, :nd])
    W, K, _ = mu.shape
    y = rd(grid).reshape(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = (y[None, None, :, None] - mu[:, :, None, :]) / np.sqrt(sig2)[:, :, None, :]          # (W, K, G, nd)
        phi = _erfc(-z / math.sqrt(2.0)).astype(np.float64) / 2.0
    out = np.empty((W, len(horizons), y.size))
    for j, h in enumerate(horizons):
        w = pi
        if h > 0:
            At = rd(A[:, :, :, :nd])
        for _ in range(h):
            nw = np.empty_like(w)
            for c in range(K):
                t = w[:, 0] * At[:, c, 0]
                for i in range(1, K):
                    t = t + w[:, i] * At[:, c, i]
                nw[:, c] = t
            w = nw
        with np.errstate(invalid="ignore"):
            f = w[:, 0, None, :] * phi[:, 0]
            for k in range(1, K):
                f = f + w[:, k, None, :] * phi[:, k]
            out[:, j] = np.mean(f, axis=2)
    return out


def make_draws(seed, W, K, nd, pad=0, with_A=True):
    """Seeded draws in the C-ABI layouts with leading dimension nd + pad; the padding columns hold NaN, so a read past nd shows.
    Variances stay >= 1e-3: every reference value is finite."""
    rng = np.random.default_rng(seed)
    ld = nd + pad
    mu = np.sort(rng.normal(2.0, 3.0, size=(W, K, ld)), axis=1)
    sig2 = 1e-3 + rng.gamma(2.0, 1.0, size=(W, K, ld))
    pi = rng.dirichlet(np.ones(K), size=(W, ld)).transpose(0, 2, 1).copy()                       # (W, K, ld)
    A = None
    if with_A:
        rows = rng.dirichlet(np.ones(K), size=(W, ld, K))                                        # [w, d, i, j]: row i sums to 1
        A = np.ascontiguousarray(rows.transpose(0, 3, 2, 1))                                     # [w, j, i, d]
    for a in (mu, sig2, pi, A):
        if a is not None:
            a[..., nd:] = np.nan
    return mu, sig2, pi, A


def make_grid(G):
    return np.array([2.0]) if G == 1 else np.linspace(-5.0, 15.0, G)
