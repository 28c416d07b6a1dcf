"""Reference, bounds and cases for the ergodic-moment tests (no GPU): the rules of hmcg_ergodic_moments[_device] in
include/hmcg_ergodic.h restated in numpy, one rounded float64 operation per step (numpy's elementwise operations are unfused),
which the per-draw columns of the library are compared against BIT FOR BIT; the same expressions in np.longdouble; and the
bounds between the two, derived here, nothing measured.

Per-draw bounds.  u = 2^-53.  Every intermediate of the GTH elimination, of x, tot and pi, and of the duration sums is a sum,
product or quotient of NON-NEGATIVE numbers (the inputs of the cases are non-negative cells; no subtraction occurs).  For such
an expression the computed value is the exact one times (1 + d_1) .. (1 + d_c), |d_i| <= u, where c counts the roundings along
the longest path: an exact input has c = 0; a sum has max(c_a, c_b) + 1 (both terms non-negative, so the larger relative error
bounds that of the sum); a product or a quotient c_a + c_b + 1.  `depth(K)` runs the very statements of `columns` on counters
with these three rules and returns the largest c over pi and over dur.  The relative error is then at most
gamma(c) = c u / (1 - c u); against the longdouble evaluation of the same expression (same count, 2^-64 per rounding) the two
errors add: gamma(c) (1 + 2^-10) covers both and the division by the reference instead of the exact value.  (For scale: the count for
pi is 6 at K = 2, 30 at K = 3 and 18 588 at K = 8 -- a product adds the counts of its factors, and the elimination nests K - 1
deep -- that is 2e-12 relative at K = 8; 3 000 random rounded matrices per K stay within 8 u.  The multiplication by
x[0] = 1 is exact and is counted all the same.)  An exact 0 (a transient
state) and a non-finite value (a reducible draw) carry no error: they must match exactly.
  m = sum_k pi_k mu_k: each term carries c_pi + 1 roundings, the K - 1 additions one each: |dm| <= gamma(c_pi + K) sum_k |pi_k mu_k|,
    the usual absolute-sum bound.
  v = within + between.  within = sum_k pi_k sig2_k, non-negative terms: gamma(c_pi + K) within.  between = sum_k pi_k e_k^2,
    e_k = mu_k - m: the computed e_k errs by de_k = |dm| (1 + u) + u |e_k| (the error of m, one subtraction), its square by
    d2_k = (2 |e_k| + de_k) de_k + u (|e_k| + de_k)^2, the term pi_k e_k^2 by pi_k [d2_k (1 + g) + g e_k^2] with
    g = gamma(c_pi + 1), the K - 1 additions and the last one gamma(K) of the sum.  Bound:
    gamma(c_pi + K + 1) (within + between) + (1 + gamma(c_pi + K + 1)) sum_k pi_k d2_k, times (1 + 2^-10) for the reference.

Pooled bounds: the library's mean = p + S1 / g and variance = (S2 - S1^2 / g) / (g - 1) over the g good draws about the pivot p
have the shape of hmcg_chain_density's, so the derivation of tests/density_cases.py holds word for word with n = g and
R = max |x - p| over the good draws: mean (g + 3) u R + u |mean|, variance (3 g + 7) 2 u R^2 (the fused multiply-add in S2
removes a rounding, the bound stays)."""
import numpy as np

from density_cases import round5

LD = np.longdouble
U = 2.0 ** -53
SLAB = 1024
ND = (1, 63, 64, 65, 255, 256, 257, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 3)
KS = tuple(range(2, 9))


def ncols(K):
    return 2 * K + 2


# ---- the rule, generic over what `+`, `*` and `/` mean --------------------------------------------------------------------------

def gth(P, one):
    """pi (a list of K) from P[i][j], i != j (row i the from-state; P[i][i] is never touched).  P is consumed."""
    K = len(P)
    for n in range(K - 1, 0, -1):
        S = P[n][0]
        for j in range(1, n):
            S = S + P[n][j]
        for i in range(n):
            P[i][n] = P[i][n] / S
        for i in range(n):
            for j in range(n):
                if i != j:
                    P[i][j] = P[i][j] + P[i][n] * P[n][j]
    x = [one]
    for j in range(1, K):
        t = x[0] * P[0][j]
        for i in range(1, j):
            t = t + x[i] * P[i][j]
        x.append(t)
    tot = x[0]
    for k in range(1, K):
        tot = tot + x[k]
    return [xk / tot for xk in x]


def durations(P, one):
    K = len(P)
    out = []
    for i in range(K):
        cells = [P[i][j] for j in range(K) if j != i]
        s = cells[0]
        for c in cells[1:]:
            s = s + c
        out.append(one / s)
    return out


def columns(mu, sig2, A, dtype=np.float64):
    """The C = 2K + 2 per-draw columns (C, n) from mu, sig2 (K, n) and A (K, K, n) in the ABI's order A[j, i, d] = draw d of
    A[i][j]; the inputs as they are (round them first for a ROUND5 call).  dtype: np.float64 (the restatement) or np.longdouble."""
    mu, sig2, A = (np.asarray(a, dtype=np.float64).astype(dtype) for a in (mu, sig2, A))
    K, n = mu.shape
    one = np.ones(n, dtype=dtype)
    cells = lambda: [[None if i == j else A[j, i].copy() for j in range(K)] for i in range(K)]
    with np.errstate(all="ignore"):
        dur = durations(cells(), one)
        pi = gth(cells(), one)
        m = pi[0] * mu[0]
        for k in range(1, K):
            m = m + pi[k] * mu[k]
        within = pi[0] * sig2[0]
        for k in range(1, K):
            within = within + pi[k] * sig2[k]
        between = None
        for k in range(K):
            e = mu[k] - m
            t = pi[k] * (e * e)
            between = t if between is None else between + t
        return np.array(pi + dur + [m, within + between])


def panel_columns(mu, sig2, A, nd=None, round5_=True, dtype=np.float64):
    """cols (W, C, nd) of a call over mu, sig2 (W, K, ld) and A (W, K, K, ld)."""
    W, K, ld = mu.shape
    nd = ld if nd is None else int(nd)
    r = round5 if round5_ else (lambda x: np.asarray(x, dtype=np.float64))
    return np.array([columns(r(mu[w, :, :nd]), r(sig2[w, :, :nd]), r(A[w, :, :, :nd]), dtype) for w in range(W)])


# ---- the rounding counts --------------------------------------------------------------------------------------------------------

class Count:
    """The number of roundings along the longest path to a non-negative value (module docstring)."""

    def __init__(self, c=0):
        self.c = c

    def __add__(self, o):
        return Count(max(self.c, o.c) + 1)

    def __mul__(self, o):
        return Count(self.c + o.c + 1)

    __truediv__ = __mul__


def depth(K):
    """(c_pi, c_dur): the largest rounding count over the K values of pi and of dur, exact inputs."""
    cells = lambda: [[None if i == j else Count() for j in range(K)] for i in range(K)]
    return max(v.c for v in gth(cells(), Count())), max(v.c for v in durations(cells(), Count()))


def gamma(c):
    return c * U / (1.0 - c * U)


REF = 1.0 + 2.0 ** -10          # the longdouble reference's own roundings, and its use as the divisor


def column_bounds(ref, mu, sig2):
    """Absolute bounds (C, n) on |restatement - ref| per cell from the longdouble columns ref (C, n) and the inputs mu, sig2
    (K, n) as the call used them.  Cells where ref is 0 or not finite get 0: they must match exactly."""
    K = mu.shape[0]
    c_pi, c_dur = depth(K)
    ref = np.asarray(ref, dtype=LD)
    mu, sig2 = np.asarray(mu, dtype=np.float64).astype(LD), np.asarray(sig2, dtype=np.float64).astype(LD)
    pi, m = ref[:K], ref[2 * K]
    out = np.zeros(ref.shape, dtype=LD)
    with np.errstate(all="ignore"):
        out[:K] = gamma(c_pi) * REF * np.abs(pi)
        out[K:2 * K] = gamma(c_dur) * REF * np.abs(ref[K:2 * K])
        dm = gamma(c_pi + K) * REF * np.abs(pi * mu).sum(axis=0)
        out[2 * K] = dm
        e = np.abs(mu - m)
        de = dm * (1.0 + U) + U * e
        d2 = (2.0 * e + de) * de + U * (e + de) ** 2
        g = gamma(c_pi + K + 1)
        out[2 * K + 1] = (g * np.abs(ref[2 * K + 1]) + (1.0 + g) * (pi * d2).sum(axis=0)) * REF
    return np.where(np.isfinite(ref) & np.isfinite(out), out, 0.0).astype(np.float64)


def solve_pi(A):
    """The stationary law of ONE matrix A[i][j] (row i the from-state) the way a caller without the library computes it:
    numpy.linalg.solve of (Q' with its last row replaced by ones) x = e_K, Q = A - diag(row sums of the off-diagonal cells)."""
    K = A.shape[0]
    off = A - np.diag(np.diag(A))
    M = (off - np.diag(off.sum(axis=1))).T.copy()
    M[-1, :] = 1.0
    b = np.zeros(K)
    b[-1] = 1.0
    return np.linalg.solve(M, b)


# ---- matrices -------------------------------------------------------------------------------------------------------------------

def nearly_reducible(K, n, seed):
    """n rounded transition matrices (n, K, K), A[d, i, j]: Dirichlet rows of mixed concentration, every third one with the
    diagonal 1 - 10^-3 .. 10^-5 and off-diagonal cells of the order 1e-4 and below, then rounded to 5 digits as CSV cells."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, K, K))
    for t in range(n):
        A = rng.dirichlet(np.full(K, rng.choice([0.05, 0.3, 1.0])), size=K)
        if t % 3 == 0:
            A = np.eye(K) * (1.0 - 10.0 ** -rng.integers(3, 6)) + A * 1e-4
        out[t] = np.rint(A * 1e5) / 1e5
    return out


def to_abi(Ad):
    """(n, K, K) matrices A[d, i, j] -> the ABI's (K, K, n) with [j, i, d]."""
    return np.ascontiguousarray(np.transpose(Ad, (2, 1, 0)))


DIRECTED = ("absorbing last", "absorbing first", "transient", "persistent", "row sums", "nan diagonal", "nan mu", "nan sig2",
            "sig2 zero", "equal mu")
# what a directed draw must give: good (every column finite) or not
DIRECTED_GOOD = {"absorbing last": False, "absorbing first": False, "transient": True, "persistent": True, "row sums": True,
                 "nan diagonal": True, "nan mu": False, "nan sig2": False, "sig2 zero": True, "equal mu": True}


def directed_good(name, K):
    """Whether a directed draw has every column finite.  At K = 2 a transient state 1 leaves state 0 absorbing."""
    return DIRECTED_GOOD.get(name, True) and not (name == "transient" and K == 2)


def directed(name, K, rng):
    """One draw (A (K, K) as A[i][j] with its diagonal filled in, mu (K,), sig2 (K,)) of the kind `name`.  All cells are
    multiples of 1e-5 or NaN, so ROUND5 leaves them as they are up to the cell rounding itself."""
    A = np.rint(rng.dirichlet(np.full(K, 1.0), size=K) * 1e5) / 1e5
    A[A == 0.0] = 1e-5
    mu = np.round(rng.standard_normal(K) + 2.0 * np.arange(K), 5)
    sig2 = np.round(0.05 + rng.gamma(2.0, 0.8, size=K), 5)
    if name == "absorbing last":                     # S == 0 in the first elimination step
        A[K - 1, :] = 0.0
        A[K - 1, K - 1] = 1.0
    elif name == "absorbing first":                  # pi = (1, 0, ..) is finite; dur[0] = +inf
        A[0, :] = 0.0
        A[0, 0] = 1.0
    elif name == "transient":                        # nobody enters the last state: an exact 0 in pi
        A[:K - 1, K - 1] = 0.0
    elif name == "persistent":                       # 1 - 1e-5 on the diagonal, 1e-5 to the next state, 0 elsewhere
        A = np.eye(K) * (1.0 - 1e-5)
        for i in range(K):
            A[i, (i + 1) % K] = 1e-5
    elif name == "row sums":                         # rows that sum to 1 +- 1e-5 after rounding
        for i in range(K):
            A[i, i] = 0.0
            A[i, i] = np.round(1.0 - A[i].sum() + (1e-5 if i % 2 else -1e-5), 5)
    elif name == "nan diagonal":
        A[np.arange(K), np.arange(K)] = np.nan
    elif name == "nan mu":
        mu[K // 2] = np.nan
    elif name == "nan sig2":
        sig2[K - 1] = np.nan
    elif name == "sig2 zero":
        sig2[:] = 0.0
    elif name == "equal mu":                         # the between part vanishes (to the rounding of m)
        mu[:] = mu[0]
    else:
        raise KeyError(name)
    return A, mu, sig2


def make_panel(seed, W, K, nd, pad=0, placed=()):
    """mu, sig2 (W, K, nd + pad), A (W, K, K, nd + pad) of generic persistent draws (diagonals 0.9 .. 0.99999, unrounded, large
    common offset in mu of window 1) with the directed draws `placed` = ((w, d, name), ..) put in; the padding alternates NaN
    and 1e300, so a read past nd changes a result.  The diagonal of A is NaN in every odd draw: it is never read."""
    rng = np.random.default_rng(seed)
    ld = nd + pad
    mu, sig2, A = np.empty((W, K, ld)), np.empty((W, K, ld)), np.empty((W, K, K, ld))
    for w in range(W):
        stay = 1.0 - 10.0 ** -rng.uniform(1.0, 5.0, size=(nd, K))
        off = rng.dirichlet(np.full(K - 1, 0.7), size=(nd, K)) * (1.0 - stay)[:, :, None]
        Ad = np.zeros((nd, K, K))
        for i in range(K):
            Ad[:, i, [j for j in range(K) if j != i]] = off[:, i, :]
            Ad[:, i, i] = stay[:, i]
        Ad[1::2, np.arange(K), np.arange(K)] = np.nan
        A[w, :, :, :nd] = to_abi(Ad)
        mu[w, :, :nd] = (rng.standard_normal((nd, K)) * 0.3 + 2.0 * np.arange(K) + (1e4 if w == 1 else 0.0)).T
        sig2[w, :, :nd] = (0.05 + rng.gamma(2.0, 0.8, size=(nd, K))).T
    for w, d, name in placed:
        a, m, s = directed(name, K, rng)
        A[w, :, :, d], mu[w, :, d], sig2[w, :, d] = a.T, m, s
    fill = np.array([np.nan, 1e300])[np.arange(pad) % 2]
    mu[:, :, nd:], sig2[:, :, nd:], A[:, :, :, nd:] = fill, fill, fill
    return mu, sig2, A


# ---- pooled over the draws ------------------------------------------------------------------------------------------------------

def pooled_reference(cols):
    """From per-draw columns (W, C, nd): n (W, 2) int64 = (good, bad), and in longdouble, two-pass about the library's pivot,
    mean and variance (W, C) over the good draws, plus R (W, C) = max |x - p| for `pooled_tolerance`."""
    cols = np.asarray(cols, dtype=np.float64)
    W, Cn, nd = cols.shape
    n = np.zeros((W, 2), dtype=np.int64)
    mean, var, R = np.full((W, Cn), np.nan, dtype=LD), np.full((W, Cn), np.nan, dtype=LD), np.zeros((W, Cn))
    for w in range(W):
        good = np.isfinite(cols[w]).all(axis=0)
        g = int(good.sum())
        n[w] = g, nd - g
        if g == 0:
            continue
        p = (cols[w, :, 0] if good[0] else np.zeros(Cn)).astype(LD)
        a = cols[w][:, good].astype(LD) - p[:, None]
        m = a.sum(axis=1) / LD(g)
        mean[w] = p + m
        if g > 1:
            var[w] = ((a - m[:, None]) ** 2).sum(axis=1) / LD(g - 1)
        R[w] = np.abs(a).max(axis=1).astype(np.float64)
    return {"n": n, "mean": mean, "variance": var, "R": R}


def pooled_tolerance(ref):
    g = ref["n"][:, :1].astype(np.float64)
    R = ref["R"]
    with np.errstate(invalid="ignore", over="ignore"):
        return {"mean": (g + 3.0) * U * R + U * np.abs(ref["mean"].astype(np.float64)), "variance": (3.0 * g + 7.0) * 2.0 * U * R * R}


def check_pooled(out, n, cols, label=""):
    """out (W, C, 2), n (W, 2) of the library against the longdouble moments of `cols` (the library's own per-draw columns):
    n exactly, NaN positions exactly, the rest within `pooled_tolerance`.  Prints and returns the worst diff / bound."""
    ref = pooled_reference(cols)
    out, n = np.asarray(out), np.asarray(n)
    assert n.dtype == np.int64 and np.array_equal(n, ref["n"]), (label, n, ref["n"])
    tol = pooled_tolerance(ref)
    worst = {}
    for i, key in enumerate(("mean", "variance")):
        g, r = out[:, :, i], ref[key]
        rf = r.astype(np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(rf)), (label, key, "NaN positions differ", g, rf)
        ok = ~np.isnan(rf)
        diff = np.abs(g[ok].astype(LD) - r[ok]).astype(np.float64)
        bound = tol[key][ok]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = float(np.max(np.where(diff == 0.0, 0.0, diff / bound))) if diff.size else 0.0
        print("%s pooled %-8s worst diff / bound = %.3g over %d cells" % (label, key, ratio, diff.size))
        assert (diff <= bound).all(), (label, key, ratio)
        worst[key] = ratio
    return worst


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_cells(got, want):
    """Two float64 arrays equal cell by cell: NaN against NaN, everything else by value and by the sign of a zero."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return bool(np.array_equal(bits(got)[ok], bits(want)[ok]))
