"""Reference, bounds and hand-made draws for the predictive-quantile tests (no GPU): the algorithm of include/hmcg_fan.h restated
in float64 numpy with math.erfc -- the range pass, round 1 on 129 points, rounds of 31 interior points, the cell choice and the
finish, every step one rounded operation in the header's order --, a long-double CDF to judge a returned quantile by, and the
two derived bounds.

Bounds (derived, not measured):
  tolF = predictive_cases.tolerance(nd, K, h_max): |computed F - exact F| at one point, the bound of the CDF entry.
  B = (hi - lo)^2 / 8 * mean_d sum_k omega_dk * 0.242 / sig2_dk: inverse linear interpolation over the last bracket.  Between lo
  and hi the chord of F misses F by at most (hi - lo)^2 / 8 * max |F''|, and F'' = sum omega f', |f'| = |z phi(z)| / sig2 <=
  0.24197 / sig2 per component (the maximum of |z phi(z)| is phi(1) = 0.24197).  q solves chord(q) = p, so |F(q) - p| <= B, plus
  the error of the two computed end values and of F_ld itself: B + 4 tolF.
  The bracket after R rounds is (hi0 - lo0) / (128 * 32^(R - 1)) wide.  Its ends are sums lo + m * step of magnitude up to
  max(|lo0|, |hi0|): each round rounds both ends (half an ulp of that magnitude each) and step (m <= 128 times half an ulp of
  step, below another ulp), and the round after divides what is left by 32, so the width is off by less than 3 ulps of
  max(|lo0|, |hi0|) however many rounds there are; the tests allow 8 R of those ulps."""
import math

import numpy as np

import predictive_cases as pc

LD = np.longdouble
SLAB = 1024
M1, M = 128, 32
_erfc = np.frompyfunc(math.erfc, 1, 1)
NAN_, UNREACHED, FLAT = 1, 2, 4

PROBS5 = (0.025, 0.16, 0.5, 0.84, 0.975)
PROBS16 = (1e-6, 1e-4, 0.005, 0.025, 0.05, 0.16, 0.25, 0.5, 0.5, 0.75, 0.84, 0.95, 0.975, 0.995, 1 - 1e-4, 1 - 1e-6)
H8 = (0, 0, 1, 2, 3, 5, 8, 12)

# The CPU table: (seed, K, nd, spread of the means, horizons, probs, rounds).  Means close together (spread 0.3: one hump) and
# well apart (spread 6: separated humps with nearly flat stretches of F between them), probabilities from 1e-6 to 1 - 1e-6.
CPU_CASES = [
    (11, 2, 300, 0.3, (0,), PROBS16, 4),
    (12, 2, 300, 6.0, (0, 12), PROBS16, 4),
    (13, 3, 1500, 1.0, (0, 1), PROBS5, 4),
    (14, 3, 200, 6.0, (0,), PROBS16, 1),
    (15, 3, 200, 6.0, (3,), PROBS16, 2),
    (16, 8, 120, 0.3, (0,), PROBS16, 6),
    (17, 8, 120, 6.0, (2, 0), PROBS5, 10),
    (18, 3, 1, 1.0, (0,), PROBS5, 3),
]


def make_draws(seed, W, K, nd, pad=0, with_A=True, spread=1.0):
    """predictive_cases.make_draws with the means scaled about their centre: spread < 1 pulls the regimes together, > 1 apart."""
    mu, sig2, pi, A = pc.make_draws(seed, W, K, nd, pad, with_A)
    mu = 2.0 + spread * (mu - 2.0)
    return mu, sig2, pi, A


def _rd(round5):
    return (lambda x: np.round(np.asarray(x, dtype=np.float64), 5)) if round5 else (lambda x: np.asarray(x, dtype=np.float64))


def omega(pi, A, h, dtype=np.float64):
    """pi A^h per draw by h successive products, k ascending: pi (K, nd), A (K, K, nd) in the ABI's order [j, i, d]."""
    w = pi.astype(dtype)
    K = w.shape[0]
    with np.errstate(invalid="ignore"):
        for _ in range(h):
            nw = np.empty_like(w)
            for c in range(K):
                t = w[0] * A[c, 0].astype(dtype)
                for i in range(1, K):
                    t = t + w[i] * A[c, i].astype(dtype)
                nw[c] = t
            w = nw
    return w


def F64(y, mu, sig2, wts):
    """The CDF at the points y (any shape) in the library's order: per draw w_0 ph_0, then w_k ph_k + F (the library fuses that
    step: one rounding fewer, inside tolF); the draws added in draw order inside a slab of 1024, the slabs in slab order; / nd."""
    y = np.asarray(y, dtype=np.float64)
    ys = y.reshape(-1)
    K, nd = mu.shape
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c = 1.0 / (1.4142135623730951 * np.sqrt(sig2))
        f = None
        for k in range(K):
            t = (ys[None, :] - mu[k][:, None]) * c[k][:, None]                     # (nd, P)
            ph = 0.5 * _erfc(-t).astype(np.float64)
            f = wts[k][:, None] * ph if k == 0 else wts[k][:, None] * ph + f
        tot = np.zeros(ys.size)
        for s in range(0, nd, SLAB):
            tot = tot + np.cumsum(f[s:s + SLAB], axis=0)[-1]
        return (tot / float(nd)).reshape(y.shape)


def Fld(y, mu, sig2, wts):
    """The same CDF with arguments, weights, products and sums in long double (wts: omega(.., LD)).  Phi is math.erfc at the
    double nearest the argument plus the first-order term of what the rounding of the argument left: erfc itself to its ulp."""
    y = np.asarray(y, dtype=LD)
    ys = y.reshape(-1)
    K, nd = mu.shape
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        tot = np.zeros(ys.size, dtype=LD)
        for k in range(K):
            sd = np.sqrt(sig2[k].astype(LD))
            t = (ys[None, :] - mu[k].astype(LD)[:, None]) / (np.sqrt(LD(2.0)) * sd[:, None])
            td = t.astype(np.float64)
            ph = 0.5 * _erfc(-td).astype(np.float64).astype(LD)
            corr = np.where(np.isfinite(td), (t - td.astype(LD)) * (np.exp(-td * td) / math.sqrt(math.pi)).astype(LD), LD(0.0))
            tot = tot + (wts[k][:, None] * (ph + corr)).sum(axis=0)
        return (tot / LD(nd)).reshape(y.shape)


def points(lo, hi, Mc):
    """y_0..y_Mc of the bracket(s) (lo, hi): step = (hi - lo) / Mc, y_m = lo + m * step, y_Mc = hi.  lo, hi (...,) -> (..., Mc + 1)."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        step = (hi - lo) / float(Mc)
        y = lo[..., None] + np.arange(Mc + 1, dtype=np.float64) * step[..., None]
    y[..., Mc] = hi
    return y


def choose(y, F, p):
    """One probability's cell of the Mc + 1 points y with values F: (lo, hi, Flo, Fhi)."""
    Mc = len(y) - 1
    with np.errstate(invalid="ignore"):
        hit = np.flatnonzero(F[1:] >= p)
    ms = int(hit[0]) + 1 if hit.size else Mc
    return y[ms - 1], y[ms], F[ms - 1], F[ms]


def finish(lo, hi, Flo, Fhi, p):
    """(q, flag) by the header's rule 5."""
    if np.isnan(Flo) or np.isnan(Fhi):
        return np.nan, NAN_
    with np.errstate(invalid="ignore", over="ignore"):
        dF = Fhi - Flo
        if not dF > 0.0:
            return lo, FLAT
        if p > Fhi:
            return hi, UNREACHED
        return lo + (hi - lo) * ((p - Flo) / dF), 0


def window_range(mu, sig2):
    """(lo0, hi0) of one window's rounded draws (K, nd)."""
    with np.errstate(invalid="ignore"):
        r = 40.0 * np.sqrt(sig2)
        lo, hi = mu - r, mu + r
    return np.fmin.reduce(lo.reshape(-1)), np.fmax.reduce(hi.reshape(-1))


def invert(Fev, lo0, hi0, probs, rounds):
    """The rounds, the cell choice and the finish for one (window, horizon); Fev(y) evaluates the CDF at an array of points.
    Returns out (n_p, 5) and flag (n_p,)."""
    n_p = len(probs)
    y = points(lo0, hi0, M1)
    F = Fev(y)
    br = [choose(y, F, p) for p in probs]
    for _ in range(1, rounds):
        ys = points(np.array([b[0] for b in br]), np.array([b[1] for b in br]), M)          # (n_p, 33)
        Fi = Fev(ys[:, 1:M])
        br = [choose(ys[i], np.concatenate(([br[i][2]], Fi[i], [br[i][3]])), probs[i]) for i in range(n_p)]
    out, flag = np.empty((n_p, 5)), np.zeros(n_p, dtype=np.int32)
    for i, (b, p) in enumerate(zip(br, probs)):
        q, flag[i] = finish(*b, p)
        out[i] = (q,) + tuple(b)
    return out, flag


def rounds_of(rounds):
    return 4 if rounds == 0 else rounds


def reference(mu, sig2, pi_end, A, probs, horizons, rounds, round5, nd=None):
    """out (W, n_h, n_p, 5), range (W, 2), flag (W, n_h, n_p) from draw arrays in the C-ABI layouts over their first nd draws."""
    rd = _rd(round5)
    nd = mu.shape[2] if nd is None else nd
    mu, sig2, pi = rd(mu[:, :, :nd]), rd(sig2[:, :, :nd]), rd(pi_end[:, :, :nd])
    At = rd(A[:, :, :, :nd]) if A is not None else None
    W = mu.shape[0]
    out = np.empty((W, len(horizons), len(probs), 5))
    rng = np.empty((W, 2))
    flag = np.zeros((W, len(horizons), len(probs)), dtype=np.int32)
    for w in range(W):
        rng[w] = window_range(mu[w], sig2[w])
        for j, h in enumerate(horizons):
            wts = omega(pi[w], At[w] if h > 0 else None, h)
            out[w, j], flag[w, j] = invert(lambda y: F64(y, mu[w], sig2[w], wts), rng[w, 0], rng[w, 1], probs, rounds_of(rounds))
    return out, rng, flag


def judge(mu, sig2, pi_end, A, horizons, round5, nd=None):
    """Per (window, horizon) what a returned quantile is judged by: Fld(y) over the rounded draws, and the curvature term
    mean_d sum_k omega_dk * 0.242 / sig2_dk of B.  Returns a function (w, j) -> (F_ld, curvature)."""
    rd = _rd(round5)
    nd = mu.shape[2] if nd is None else nd
    mu, sig2, pi = rd(mu[:, :, :nd]), rd(sig2[:, :, :nd]), rd(pi_end[:, :, :nd])
    At = rd(A[:, :, :, :nd]) if A is not None else None

    def at(w, j):
        h = horizons[j]
        wts = omega(pi[w], At[w] if h > 0 else None, h, LD)
        with np.errstate(divide="ignore", invalid="ignore"):
            curv = float((wts * (LD(0.242) / sig2[w].astype(LD))).sum(axis=0).mean())
        return (lambda y: Fld(y, mu[w], sig2[w], wts)), curv
    return at


def tolF(nd, K, horizons):
    return pc.tolerance(nd, K, max(horizons))


def ulp_of_range(rng):
    return float(np.spacing(np.max(np.abs(rng))))


def check_block(out, rng, flag, probs, horizons, rounds, nd, K, at, label=""):
    """The properties every returned block must have, against the long-double CDF `at` (judge(...)): lo <= q <= hi, the bracket
    width, |F_ld(q) - p| <= B + 4 tolF, F_ld(lo) <= p + tolF and F_ld(hi) >= p - tolF where the flag is 0.  Items whose flag
    is NAN are checked for a NaN quantile only.  Returns the largest |F_ld(q) - p| / bound met."""
    R = rounds_of(rounds)
    tol = tolF(nd, K, horizons)
    worst = 0.0
    W, n_h, n_p = flag.shape
    for w in range(W):
        width = (rng[w, 1] - rng[w, 0]) / (128.0 * 32.0 ** (R - 1))
        for j in range(n_h):
            F, curv = at(w, j)
            o = out[w, j]
            ok = (flag[w, j] & NAN_) == 0
            assert np.isnan(o[~ok, 0]).all(), (label, w, j)
            if not ok.any():
                continue
            q, lo, hi = o[ok, 0], o[ok, 1], o[ok, 2]
            p = np.asarray(probs, dtype=np.float64)[ok]
            assert (lo <= q).all() and (q <= hi).all(), (label, w, j, o)
            assert (np.abs((hi - lo) - width) <= 8 * R * ulp_of_range(rng[w])).all(), (label, w, j, hi - lo, width)
            Fl, Fh = (F(v).astype(np.float64) for v in (lo, hi))
            B = (hi - lo) ** 2 / 8.0 * curv
            # a FLAT last cell is an unreached p too: Phi has saturated below hi0 and no F climbs to p (the header's rule 5
            # tests the flat cell first), so F(hi) >= p is asked where neither bit is set
            reach = (flag[w, j][ok] & (UNREACHED | FLAT)) == 0
            err = np.abs(F(q) - p.astype(LD)).astype(np.float64)
            plain = flag[w, j][ok] == 0
            if plain.any():
                ratio = float(np.max(err[plain] / (B[plain] + 4.0 * tol)))
                worst = max(worst, ratio)
                assert ratio <= 1.0, (label, w, j, err, B, tol)
            assert (Fl <= p + tol).all(), (label, w, j, Fl, p)
            assert (Fh[reach] >= p[reach] - tol).all(), (label, w, j, Fh, p)
    return worst
