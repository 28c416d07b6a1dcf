"""Reference, derived bounds and case table for the predictive-score tests (no GPU): the formulas of include/hmcg_score.h in
numpy -- the argument t, erf and exp (scipy / numpy) in float64, every sum, weight and product in np.longdouble -- over the
used draws of a thinned call.

    a(m, S2) = m erf(m / sqrt(2 S2)) + sqrt(S2) sqrt(2 / pi) exp(-m^2 / (2 S2)),   a(m, 0) = |m|
    e_abs  = (1 / n_u)   sum_c omega_c a(y - mu_c, sig2_c)
    e_pair = (1 / n_u^2) sum_c sum_c' omega_c omega_c' a(mu_c - mu_c', sig2_c + sig2_c')
    crps = e_abs - e_pair / 2,   pit = F(y) (fan_cases.Fld),   pdf = F'(y)

Bounds (derived, not measured).  Every term of e_abs and e_pair is >= 0, and a >= max(|m|, 0.79 sqrt(S2)): m erf(t) >= 0 and
a(0, S2) = 0.798 sqrt(S2) is the minimum over m.  So the error of a term is relative to the term: the device's steps are m, S2,
sqrt, the product, the reciprocal and t (3 ulps of t at most), erf (whose relative condition t erf'(t) / erf(t) is <= 1), t * t
and exp (2 t^2 exp(-t^2) <= 0.74, times 0.798 sqrt(S2) <= 1.01 a), two products and a sum: under the 32 * 2^-52 per term that
predictive_cases.tolerance takes, counted twice because the reference evaluates t, erf and exp in float64 too (2 c = 64).  The
weights are non-negative, so a sum of such terms is off by the terms' bound plus one ulp53 per addition a term passes through,
L1 and L2 below from the order the header fixes, plus the omega recurrences against long double (K h per weight; a pair
term has two):
    tol1 = (64 + L1 + 2 K h_max) 2^-52,   L1 = (K - 1) + min(n_u, 1024) + ceil(n_u / 1024)
    tol2 = (64 + L2 + 4 K h_max) 2^-52,   L2 = N + 2 + 6 + 3 + ceil(ceil(N / 256) / 2),   N = n_u K
    |e_abs - ref| <= tol1 E1,  |e_pair - ref| <= tol2 E2,  |crps - ref| <= tol1 E1 + tol2 E2 / 2   (E1, E2 the reference's)
    |pit - ref| <= predictive_cases.tolerance(n_u, K, h_max), the bound of the CDF entry
    |pdf - ref| <= tol1 * peak,  peak = (1 / n_u) sum_c omega_c / sqrt(2 pi sig2_c): the density's terms are relative to their
    value at the mode, not at y (the absolute error of exp(-t^2) is 2 t^2 exp(-t^2) <= 0.74 ulps of 1)."""
import math

import numpy as np
from scipy.special import erf as _erf

import fan_cases as fc
import predictive_cases as pc

LD = np.longdouble
FIELDS = ("crps", "e_abs", "e_pair", "pit", "pdf")
DRAWS_DEFAULT = 4096
TP = 256                                 # components per tile of the pair pass; a block owns two rows of tiles
SLAB = 1024
C_TERM = 32.0
H8 = (0, 0, 1, 2, 3, 5, 8, 12)


def thinning(nd, stride):
    """(stride, n_u) of a call: stride 0 is the smallest stride with n_u <= 4096."""
    if stride == 0:
        stride = max(1, -(-nd // DRAWS_DEFAULT))
    return stride, -(-nd // stride)


def tiles(N):
    return -(-N // TP)


def blocks(N):
    return (tiles(N) + 1) // 2


def row_pairing(nT):
    """Per block the rows of tiles it takes: b and nT - 1 - b, once where they are equal."""
    return [[b] if b == nT - 1 - b else [b, nT - 1 - b] for b in range((nT + 1) // 2)]


def work_doubles(n_u, K, n_h):
    N = n_u * K
    return N * (2 + n_h) + (-(-n_u // SLAB)) * 3 * n_h + blocks(N) * n_h


def L1(K, n_u):
    return (K - 1) + min(n_u, SLAB) + (-(-n_u // SLAB))


def L2(K, n_u):
    N = n_u * K
    return N + 2 + 6 + 3 + blocks(N)


def tol1(K, n_u, h_max):
    return (2.0 * C_TERM + L1(K, n_u) + 2 * K * h_max) * 2.0 ** -52


def tol2(K, n_u, h_max):
    return (2.0 * C_TERM + L2(K, n_u) + 4 * K * h_max) * 2.0 ** -52


def a_ld(m, S2):
    """a(m, S2) for long-double arrays: t, erf and exp in float64 (t from the doubles nearest m and S2: its few ulps are inside
    the second c of the bound), the products and the sum in long double."""
    m, S2 = np.asarray(m, dtype=LD), np.asarray(S2, dtype=LD)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s64 = np.sqrt(S2.astype(np.float64))
        t = m.astype(np.float64) / (1.4142135623730951 * s64)
        a = m * _erf(t) + (np.sqrt(LD(2.0) / LD(np.pi)) * s64) * np.exp(-(t * t))
    return np.where(S2 == 0, np.abs(m), a)


def pair_sums(m, v, ws, chunk=1 << 20):
    """sum_c sum_c' w_c w_c' a(m_c - m_c', v_c + v_c') for each weight vector of ws, by the symmetry: the diagonal once, every
    pair above it twice.  Rows in chunks, so memory stays bounded."""
    N = m.size
    m, v = m.astype(LD), v.astype(LD)
    out = [LD(0.0) for _ in ws]
    rows = max(1, chunk // N)
    for i0 in range(0, N, rows):
        i1 = min(N, i0 + rows)
        sq = a_ld(m[i0:i1, None] - m[None, i0:i1], v[i0:i1, None] + v[None, i0:i1])
        sq = np.triu(sq, 1) * 2 + np.diag(np.diag(sq))
        rest = a_ld(m[i0:i1, None] - m[None, i1:], v[i0:i1, None] + v[None, i1:]) if i1 < N else None
        for j, w in enumerate(ws):
            r = sq @ w[i0:i1]
            if rest is not None:
                r = r + 2 * (rest @ w[i1:])
            out[j] = out[j] + (w[i0:i1] * r).sum()
    return out


def reference(mu, sig2, pi_end, A, yreal, horizons, stride, round5, nd=None):
    """ref (W, n_h, 5) in float64 and bound (W, n_h, 5) from draw arrays in the C-ABI layouts over every stride-th of their first
    nd draws; yreal (n_h, W)."""
    rd = fc._rd(round5)
    nd = mu.shape[2] if nd is None else nd
    st, n_u = thinning(nd, stride)
    mu, sig2, pi = rd(mu[:, :, :nd:st]), rd(sig2[:, :, :nd:st]), rd(pi_end[:, :, :nd:st])
    At = rd(A[:, :, :, :nd:st]) if A is not None else None
    W, K, _ = mu.shape
    h_max = max(horizons)
    t1, t2, tF = tol1(K, n_u, h_max), tol2(K, n_u, h_max), pc.tolerance(n_u, K, h_max)
    ref, bound = np.empty((W, len(horizons), 5)), np.empty((W, len(horizons), 5))
    for w in range(W):
        m, v = mu[w].T.reshape(-1), sig2[w].T.reshape(-1)                      # component c = u K + k
        wts = [fc.omega(pi[w], At[w] if h > 0 else None, h, LD) for h in horizons]
        pairs = pair_sums(m, v, [x.T.reshape(-1) for x in wts])
        for j in range(len(horizons)):
            y = yreal[j, w]
            om = wts[j].T.reshape(-1)
            E2 = pairs[j] / (LD(n_u) * LD(n_u))
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                E1 = (om * a_ld(LD(y) - m.astype(LD), v)).sum() / LD(n_u)
                pit = fc.Fld(np.array([y]), mu[w], sig2[w], wts[j])[0]
                sd = np.sqrt(v.astype(LD))
                z = ((LD(y) - m.astype(LD)) / sd).astype(np.float64)
                dens = om * np.exp(-0.5 * z * z).astype(LD) / (sd * np.sqrt(LD(2.0) * LD(np.pi)))
                pdf = dens.sum() / LD(n_u)
                peak = float((om / (sd * np.sqrt(LD(2.0) * LD(np.pi)))).sum() / LD(n_u))
            ref[w, j] = (float(E1 - E2 / 2), float(E1), float(E2), float(pit), float(pdf))
            bound[w, j] = (t1 * float(E1) + 0.5 * t2 * float(E2), t1 * float(E1), t2 * float(E2), tF, t1 * peak)
    return ref, bound


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the items whose reference is finite; where it is NaN the value must be NaN too."""
    got, ref = np.asarray(got), np.asarray(ref)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (got, ref)
    if nan.all():
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - ref) / bound
    r = np.where(np.abs(got - ref) == 0.0, 0.0, r)
    return float(np.max(r[~nan]))


def crps_normal(y, mu, sd):
    """Closed form for one normal: sd [z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt(pi)]."""
    z = (y - mu) / sd
    return sd * (z * math.erf(z / math.sqrt(2.0)) + 2.0 * math.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi) - 1.0 / math.sqrt(math.pi))


def used_counts(K):
    """Used-draw counts at which the kernels take another path: one draw; N = n_u K on both sides of the pair kernel's tile
    edge (256 components) and of one block's row share (two rows of tiles, 512 components); both sides of the linear pass's slab."""
    return (1, TP // K, TP // K + 1, 2 * TP // K, 2 * TP // K + 1, SLAB - 1, SLAB + 1)


NEW_KS = (4, 5, 6, 7)                    # the K between: a draw's components straddle the 256-component tile edge at 5, 6, 7
# horizon tuples of the K = 4..7 cases: every length the first table lacks, so that score_pair_kernel<2|4|5|6|7> run from here
NEW_HZS = ((0, 12), (0, 1, 2, 12), (0, 1, 2, 3, 12), (0, 0, 1, 3, 5, 12), (0, 1, 2, 3, 5, 8, 12))
# The long-double reference costs W N^2 evaluations of a(m, S2), N = n_u K.  The largest of the K in {2, 3, 8} table is K = 8 at
# 1 025 used draws in one window: no case may cost more.
PAIR_BUDGET = (8 * (SLAB + 1)) ** 2


def pair_cost(K, n_u, W):
    return W * (n_u * K) ** 2


def _gpu_cases():
    """(K, n_u, stride, pad, round5, horizons, W): K in {2, 3, 8} crossed with used_counts(K), the other options dealt
    round-robin; then K = 4..7 crossed with used_counts(K) and the horizon tuples of NEW_HZS, dealt the same way -- a case whose
    reference would exceed PAIR_BUDGET runs one window, and is dropped if it still does (none is: every K keeps its slab edges)."""
    strides, pads, r5 = (1, 2, 3), (0, 5), (True, False)
    hzs, Ws = ((0,), (0, 1, 12), H8), (1, 3)
    out, i = [], 0
    for K in (2, 3, 8):
        for n_u in used_counts(K):
            out.append((K, n_u, strides[i % 3], pads[i % 2], r5[(i // 2) % 2], hzs[(i + i // 3) % 3], Ws[(i // 3) % 2]))
            i += 1
    i = 0
    for K in NEW_KS:
        for n_u in used_counts(K):
            W = Ws[(i // 3) % 2]
            W = W if pair_cost(K, n_u, W) <= PAIR_BUDGET else 1
            if pair_cost(K, n_u, W) <= PAIR_BUDGET:
                out.append((K, n_u, strides[i % 3], pads[i % 2], r5[(i // 2) % 2], NEW_HZS[i % 5], W))
            i += 1
    return out


GPU_CASES = _gpu_cases()
DEFAULT_CASE = (2, 8209)                 # stride 0 at nd = 8209: stride 3, n_u = 2737, 1.5e7 pair terms


def nd_of(n_u, stride):
    """A draw count that leaves n_u used draws under `stride`: not a multiple of it, and at stride 3 with a draw behind the last
    used one."""
    return (n_u - 1) * stride + 1 + int(stride > 2 and n_u > 1)


def make_yreal(mu, sig2, n_h, nd, seed):
    """yreal (n_h, W), dealt round-robin over (window, horizon): a value inside the law, an unknown one (NaN) and one 40 of the
    largest standard deviations past the largest mean (pit exactly 1, crps about y - mean) or below the smallest (pit 0)."""
    W = mu.shape[0]
    rng = np.random.default_rng(seed)
    y = np.empty((n_h, W))
    for j in range(n_h):
        for w in range(W):
            kind = (j + w) % 4
            far = 40.0 * math.sqrt(float(np.max(sig2[w, :, :nd]))) + 1.0
            y[j, w] = (rng.normal(2.0, 3.0), np.nan, float(np.max(mu[w, :, :nd])) + far, float(np.min(mu[w, :, :nd])) - far)[kind]
    if n_h * W == 1:
        y[0, 0] = 2.5
    return y
