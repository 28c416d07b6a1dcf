"""Reference, tolerance, cases and launcher binding for the tests of the correlation kernels (no GPU): csrc/moments.hip's
draw_moments_kernel<PPT> (the pair table of a window's rounded draws about its first draw) and corr_finalize_kernel (the
Pearson matrix from that table), which make extras.corr.

Binding.  libhmcgibbs.so is linked with default visibility, so the launchers of csrc/moments.hpp are exported under their
Itanium names (SYMBOLS); `MomentsArgs` mirrors the struct (tests/test_corr_cases.py holds size and offsets to the header).  A
test hands the kernels buffers of its own and owns the moment table between the two launches.  Both launchers are called with
a NULL stream: the caller synchronises the device before and after.

`reference`: x' = round5(x), p = x' of draw 0, a = x' - p the fp64 subtraction the kernel defines; from there np.longdouble:
P_ij = sum a_i a_j, S_i = sum a_i, c_ij = P_ij - S_i S_j / n, r_ij = c_ij / sqrt(c_ii c_jj), diagonal 1 where c_ii > 0.

Tolerance, derived from the shape of the kernels' computation, nothing measured.  u = 2^-53, n draws (n <= 4096 is assumed),
a exact in both computations, A_ij = sum |a_i a_j|, B_i = sum |a_i|.
  Pair table.  Every pair is ONE serial chain of n fused multiply-adds in draw order, whatever the tiles and the blocks of the
    run (the accumulator travels through `mom` unrounded; the padding of the last tile adds fma(0, 0, s) = s exactly): n
    roundings, |dP_ij| <= n u / (1 - n u) A_ij <= (n + 1) u A_ij.  A sum is the pair with the constant-one column: fma(a, 1, s),
    the first of them exact (s = 0), |dS_i| <= (n - 1) u / (1 - (n - 1) u) B_i <= (n + 1) u B_i.  The count is the pair of the
    one column with itself: exactly n.
  Covariance c_ij = fl(P_ij - fl(fl(S_i S_j) / n)).  The two sums carry (n - 1) u each to first order, the product and the
    quotient one rounding each: 2 n u B_i B_j / n; the subtraction rounds its result, at most u (A_ij + B_i B_j / n); with dP:
    (n + 1) u A_ij + (2 n + 1) u B_i B_j / n to first order.  E_ij = (2 n + 4) u (A_ij + B_i B_j / n) leaves 3 u of both terms
    for what is second order in n u (below 2^-30 u for n <= 4096) and for the long-double reference's own sums (n 2^-64 =
    n 2^-11 u <= 2 u).
  Correlation r_ij = fl(c_ij / fl(fl(sqrt c_ii) fl(sqrt c_jj))): with c'_ii = c_ii (1 + e_i), |e_i| <= rho_i = E_ii / c_ii,
    r' = (c_ij + e_ij) / sqrt(c_ii c_jj) G,  G = (1 + e_i)^(-1/2) (1 + e_j)^(-1/2) (1 + t), |t| <= 4 u / (1 - 4 u): two square
    roots, one product, one quotient (the reference's own 2^-64 roundings are taken from the second-order factor).  To first order
        |dr_ij| <= E_ij / sqrt(c_ii c_jj) + |r_ij| (rho_i / 2 + rho_j / 2 + 4 u) = F_ij.
    Second order: under the guard rho <= 2^-10, |(1 + e)^(-1/2) - 1| <= rho / 2 (1 + rho), so |G - 1| <= s (1 + s) with
    s <= (rho_i / 2 + rho_j / 2 + 4 u) (1 + 2^-10) <= 2^-10 (1 + 2^-9); then |dr| <= E_ij / D (1 + s (1 + s)) + |r| s (1 + s)
    <= F_ij (1 + 2^-10) (1 + 2^-10 (1 + 2^-8)) < F_ij (1 + 2^-8).  Bound: F_ij (1 + 2^-8).  |r| <= 1 in exact arithmetic, so the
    clamp to [-1, 1] can only reduce the error.
  Guard.  A cell is held to the bound only where max(rho_i, rho_j) <= 2^-10.  The guard is a condition on the reference's own
    magnitudes, no measurement; a column that is constant after rounding has c_ii = 0 and lies outside it (its cells are NaN in
    the reference and must be NaN).  Any cell, inside or outside: NaN exactly where the reference is NaN, |r| <= 1, r_ij and
    r_ji the same bits, a diagonal of exactly 1 where c_ii > 0.

`finalize_restated` is corr_finalize_kernel in fp64, operation for operation: P - (Si * Sj) / n, sqrt * sqrt, the quotient,
the clamp, the diagonal rule.  No product feeds an addition or a subtraction directly (the quotient and the square root stand
between), so -ffp-contract=on has nothing to fuse; the kept assembly of the moments unit shows v_mul_f64 for Si * Sj and for the
product of the roots, each followed by the division's own v_div_scale / v_fma / v_div_fmas / v_div_fixup sequence, and no
fused multiply-add outside the division and square-root expansions.  Both expansions are correctly rounded, as numpy's are.
`stand_in` accumulates the pair table serially in fp64 with two roundings a step (numpy has no fma): its pair table is held to
2 n u A_ij, and its correlations to the bound above, which covers (2 n + 1) u A_ij."""
import ctypes as C

import numpy as np

from density_cases import LD, U, round5

SYMBOLS = {
    "launch_moments": "_ZN9hmcg_host14launch_momentsERKNS_11MomentsArgsEP12ihipStream_t",
    "launch_corr_finalize": "_ZN9hmcg_host20launch_corr_finalizeEPKdPdiiP12ihipStream_t",
    "moments_stride": "_ZN9hmcg_host14moments_strideEi",
    "corr_columns": "_ZN9hmcg_host12corr_columnsEi",
}
MOM_TD, MOM_NT = 64, 256                     # draws per LDS tile, threads per window (csrc/moments.hip)
MAXK = 8
PPT_OF_K = {2: 1, 3: 1, 4: 2, 5: 4, 6: 8, 7: 16, 8: 16}
ND_EDGES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 200)
KINDS = ("plain", "outlier", "collinear", "duplicate", "negated", "sticky", "constant")
GUARD = 2.0 ** -10
SECOND_ORDER = 1.0 + 2.0 ** -8
N_MAX = 4096                                 # the derivation's assumption on n


class MomentsArgs(C.Structure):
    """hmcg_host::MomentsArgs (csrc/moments.hpp)."""
    _fields_ = [("mu", C.c_void_p), ("sig2", C.c_void_p), ("pi_end", C.c_void_p), ("A", C.c_void_p), ("fcast", C.c_void_p),
                ("mom", C.c_void_p), ("nd", C.c_longlong), ("nd_ld", C.c_longlong), ("W", C.c_int), ("K", C.c_int), ("H", C.c_int),
                ("first", C.c_bool)]


def corr_columns(K):
    return 3 * K + K * K + 1


def n_pairs(K):
    NCp = corr_columns(K) + 1
    return NCp * (NCp + 1) // 2


def moments_stride(K):
    return corr_columns(K) + n_pairs(K)


def ppt_of(K):
    """The instantiation launch_moments picks: the smallest of the compiled pairs-per-thread that holds ceil(NP / 256)."""
    need = (n_pairs(K) + MOM_NT - 1) // MOM_NT
    return min(p for p in (1, 2, 4, 8, 16) if p >= need)


def pair_index(i, j, n):
    """moments.hip's pair_index: the number of (i, j), i <= j, in the row-major upper triangle of an n x n table."""
    return i * (2 * n - i + 1) // 2 + (j - i)


def pair_decode(pr, NCp):
    """The kernel's decode loop: pair number -> (i, j)."""
    i, rem = 0, pr
    while rem >= NCp - i:
        rem -= NCp - i
        i += 1
    return i, i + rem


def bind(lib):
    """Set the argument and result types of the four symbols on the loaded library; returns them by their short names."""
    f = {k: getattr(lib, v) for k, v in SYMBOLS.items()}
    f["launch_moments"].restype = C.c_int
    f["launch_moments"].argtypes = [C.POINTER(MomentsArgs), C.c_void_p]
    f["launch_corr_finalize"].restype = C.c_int
    f["launch_corr_finalize"].argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    f["moments_stride"].restype = C.c_size_t
    f["moments_stride"].argtypes = [C.c_int]
    f["corr_columns"].restype = C.c_int
    f["corr_columns"].argtypes = [C.c_int]
    return f


def launch(lib, mu, sig2, pi_end, A, fcast, mom_ptr, nd, nd_ld, W, K, H, first):
    """launch_moments on device addresses (integers), NULL stream.  Raises on a HIP error."""
    a = MomentsArgs(mu, sig2, pi_end, A, fcast, mom_ptr, nd, nd_ld, W, K, H, bool(first))
    rc = bind(lib)["launch_moments"](C.byref(a), None)
    if rc != 0:
        raise RuntimeError("launch_moments: hipError %d" % rc)


def finalize(lib, mom_ptr, corr_ptr, W, K):
    """launch_corr_finalize on device addresses, NULL stream."""
    rc = bind(lib)["launch_corr_finalize"](mom_ptr, corr_ptr, W, K, None)
    if rc != 0:
        raise RuntimeError("launch_corr_finalize: hipError %d" % rc)


# ---------------------------------------------------------------- layouts ----
def columns(mu, sig2, pi_end, A, fcast):
    """(W, NC, ld): mu | sig2 | pi | vec(A) | first forecast, from the ABI's arrays (draw index last, fcast (W, 2H, ld))."""
    W, ld = mu.shape[0], mu.shape[-1]
    return np.concatenate([mu.reshape(W, -1, ld), sig2.reshape(W, -1, ld), pi_end.reshape(W, -1, ld), A.reshape(W, -1, ld),
                           fcast.reshape(W, -1, ld)[:, :1]], axis=1)


def unpack_mom(mom, NC):
    """One window's table [NC pivots | NP pairs] -> (pivots (NC,), the symmetric (NC + 1) x (NC + 1) pair matrix)."""
    NCp = NC + 1
    iu = np.triu_indices(NCp)                 # row-major upper triangle: pair_index's order
    P = np.empty((NCp, NCp), dtype=mom.dtype)
    P[iu] = mom[NC:NC + NCp * (NCp + 1) // 2]
    P[(iu[1], iu[0])] = P[iu]
    return mom[:NC].copy(), P


# -------------------------------------------------------------- reference ----
def prepare(cols, n):
    """cols (W, NC, ld) -> x' (W, NC, n), p (W, NC), a = x' - p in fp64."""
    xr = round5(np.asarray(cols, dtype=np.float64)[:, :, :int(n)])
    p = xr[:, :, 0].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        a = xr - p[:, :, None]
    return xr, p, a


def reference(cols, n):
    """The long-double reference of a (W, NC, ld) block over its first n draws: r (W, NC, NC), c, P (pairs of the columns),
    S, the pivots p, and the magnitudes A (W, NC, NC), B (W, NC) of the bound."""
    n = int(n)
    _, p, a = prepare(cols, n)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        aL = a.astype(LD)
        P = np.einsum("wid,wjd->wij", aL, aL)
        S = aL.sum(axis=2)
        c = P - S[:, :, None] * S[:, None, :] / LD(n)
        d = np.sqrt(np.einsum("wii->wi", c))
        r = c / (d[:, :, None] * d[:, None, :])
        r = np.where(r > 1, LD(1), np.where(r < -1, LD(-1), r))
        W, NC = p.shape
        for w in range(W):
            for i in range(NC):
                if c[w, i, i] > 0:
                    r[w, i, i] = 1
        absa = np.abs(a)
        A = np.einsum("wid,wjd->wij", absa, absa)
        B = absa.sum(axis=2)
    return {"r": r, "c": c, "P": P, "S": S, "p": p, "A": A, "B": B, "n": n}


def tolerance(ref):
    """{"pair", "sum": the table's bounds; "corr": the per-cell bound (W, NC, NC); "rho" (W, NC); "guard": the cells held to
    "corr"} (module docstring)."""
    n = float(ref["n"])
    assert ref["n"] <= N_MAX
    A, B = ref["A"], ref["B"]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        E = (2.0 * n + 4.0) * U * (A + B[:, :, None] * B[:, None, :] / n)
        cd = np.einsum("wii->wi", ref["c"]).astype(np.float64)
        rho = np.einsum("wii->wi", E) / cd
        D = np.sqrt(cd[:, :, None] * cd[:, None, :])
        absr = np.abs(ref["r"].astype(np.float64))
        F = E / D + absr * (rho[:, :, None] / 2.0 + rho[:, None, :] / 2.0 + 4.0 * U)
        guard = np.maximum(rho[:, :, None], rho[:, None, :]) <= GUARD           # False where rho is NaN or infinite
    return {"pair": (n + 1.0) * U * A, "sum": (n + 1.0) * U * B, "corr": F * SECOND_ORDER, "rho": rho, "guard": guard}


def constant_columns(cols, n):
    """(W, NC) bool: the column is constant after rounding over its first n draws (or holds a non-finite value)."""
    xr, _, a = prepare(cols, n)
    return ~(np.isfinite(a).all(axis=2) & (a != 0.0).any(axis=2))


def finalize_restated(mom, NC):
    """corr_finalize_kernel on one window's table in fp64, operation for operation: (NC, NC)."""
    _, P = unpack_mom(np.asarray(mom, dtype=np.float64), NC)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        n = P[NC, NC]
        S = P[:NC, NC]
        c = P[:NC, :NC] - (S[:, None] * S[None, :]) / n
        cd = np.diag(c).copy()
        sq = np.sqrt(cd)
        r = c / (sq[:, None] * sq[None, :])
        r = np.where(r > 1.0, 1.0, np.where(r < -1.0, -1.0, r))
        r[np.arange(NC), np.arange(NC)] = np.where(cd > 0.0, 1.0, np.diag(r))
    return r


def stand_in(cols, n):
    """An fp64 stand-in of the two kernels: (W, stride) tables accumulated serially in draw order, two roundings a step, and
    finalize_restated of them (W, NC, NC)."""
    _, p, a = prepare(cols, n)
    W, NC = p.shape
    NCp = NC + 1
    iu = np.triu_indices(NCp)
    mom = np.empty((W, NC + len(iu[0])))
    corr = np.empty((W, NC, NC))
    with np.errstate(invalid="ignore", over="ignore"):
        for w in range(W):
            acc = np.zeros((NCp, NCp))
            for d in range(int(n)):
                v = np.append(a[w, :, d], 1.0)
                acc = acc + v[:, None] * v[None, :]
            mom[w, :NC] = p[w]
            mom[w, NC:] = acc[iu]
            corr[w] = finalize_restated(mom[w], NC)
    return mom, corr


# ------------------------------------------------------------------ checks ---
def check_table(mom, ref, label="", fused=True):
    """The pair tables (W, stride) against the reference: pivots array_equal, the count exactly n, every pair within
    (n + 1) u A_ij and every sum within (n + 1) u B_i (the stand-in, fused=False: twice n u), NaN positions exactly.  Prints and
    returns the worst diff / bound of pairs and sums."""
    W, NC = ref["p"].shape
    tol = tolerance(ref)
    n = ref["n"]
    k = 1.0 if fused else 2.0 * n / (n + 1.0)
    worst = {"pair": 0.0, "sum": 0.0}
    for w in range(W):
        piv, P = unpack_mom(np.asarray(mom[w], dtype=np.float64), NC)
        assert np.array_equal(piv, ref["p"][w], equal_nan=True), (label, w, "pivots")
        assert P[NC, NC] == float(n), (label, w, "count", P[NC, NC])
        for key, g, r, b in (("pair", P[:NC, :NC], ref["P"][w], k * tol["pair"][w]), ("sum", P[:NC, NC], ref["S"][w], k * tol["sum"][w])):
            rf = r.astype(np.float64)
            assert np.array_equal(np.isnan(g), np.isnan(rf)), (label, w, key, "NaN positions differ")
            ok = np.isfinite(rf)
            assert np.array_equal(g[~ok], rf[~ok], equal_nan=True), (label, w, key, "infinities differ")
            if not ok.any():
                continue
            diff = np.abs(g[ok].astype(LD) - r[ok]).astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = float(np.max(np.where(diff == 0.0, 0.0, diff / b[ok])))
            assert (diff <= b[ok]).all(), (label, w, key, float(diff.max()), ratio)
            worst[key] = max(worst[key], ratio)
    print("%s table: worst diff/bound pairs %.3g, sums %.3g" % (label, worst["pair"], worst["sum"]))
    return worst


def check(got_corr, ref, label="", cap=None, constant=None):
    """got_corr (W, NC, NC) against the reference.  Every cell: NaN exactly where the reference is NaN, |r| <= 1, the same bits
    as its transpose, a diagonal of exactly 1 where c_ii > 0.  Cells inside the guard: within the derived bound (min(bound, cap)
    with a cap).  Cells outside it: with a cap (draws the test did not make) within the cap; without one they must belong to a
    column of `constant` (W, NC; default: no column), i.e. be NaN already.  Prints and returns the worst diff / bound."""
    g = np.asarray(got_corr, dtype=np.float64)
    r = ref["r"]
    assert g.shape == r.shape, (label, g.shape, r.shape)
    tol = tolerance(ref)
    rf = r.astype(np.float64)
    assert np.array_equal(np.isnan(g), np.isnan(rf)), (label, "NaN positions differ")
    fin = ~np.isnan(rf)
    assert (np.abs(g[fin]) <= 1.0).all(), (label, "|r| > 1")
    assert np.array_equal(g, np.swapaxes(g, 1, 2), equal_nan=True), (label, "not symmetric")
    cd = np.einsum("wii->wi", ref["c"])
    dg = np.einsum("wii->wi", g)
    assert (dg[cd > 0] == 1.0).all(), (label, "diagonal")
    guard = tol["guard"] & fin
    out = fin & ~tol["guard"]
    if cap is None:
        const = np.zeros(cd.shape, dtype=bool) if constant is None else constant
        allowed = const[:, :, None] | const[:, None, :]
        assert not (~tol["guard"] & ~allowed).any(), (label, "the guard excludes a cell of a live column", float(np.nanmax(tol["rho"])))
        assert not out.any(), (label, "a finite cell outside the guard")
    else:
        assert (np.abs(g[out].astype(LD) - r[out]) <= cap).all(), (label, "outside the guard, beyond the cap")
    if not guard.any():
        print("%s corr: no finite cell" % label)
        return 0.0
    diff = np.abs(g[guard].astype(LD) - r[guard]).astype(np.float64)
    bound = tol["corr"][guard]
    if cap is not None:
        bound = np.minimum(bound, cap)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.max(np.where(diff == 0.0, 0.0, diff / bound)))
    print("%s corr: max |diff| = %.3e, bound there %.3e (bounds %.1e .. %.1e), largest rho %.1e, worst diff/bound = %.3g"
          % (label, float(diff.max()), float(bound[np.argmax(diff)]), float(bound.min()), float(bound.max()),
             float(np.max(tol["rho"][np.isfinite(tol["rho"])], initial=0.0)), ratio))
    assert (diff <= bound).all(), (label, float(diff.max()), ratio)
    return ratio


# ------------------------------------------------------------------- cases ---
def make_case(seed, W, K, H, nd, pad, kind):
    """(mu, sig2, pi_end, A, fcast) in the ABI's layouts -- (W, K, ld), (W, K, ld), (W, K, ld), (W, K * K, ld), (W, 2H, ld), ld =
    nd + pad --, NaN in the pad draws beyond nd and in every forecast column other than column 0 (finite outputs then prove
    them unread).  The kinds change columns of the plain case:
      outlier    mu_0's first draw 30 sd from the rest; sig2_0 at 1e4 with a spread of 1e-2
      collinear  mu_1 = 0.5 mu_0 + 1e-4 noise
      duplicate  mu_1 = mu_0;  negated: mu_1 = -mu_0 (exactly opposite after rounding: rint is odd)
      sticky     pi_0 = 1.0 with min(3, nd - 1) draws of 0.99999
      constant   sig2_1 = 0.7 + 1e-7 noise: constant after rounding"""
    assert kind in KINDS, kind
    rng = np.random.default_rng(seed)
    ld = nd + pad
    KK = K * K

    def blank(ncol):
        return np.full((W, ncol, ld), np.nan)

    mu, sig2, pi_end, A, fcast = blank(K), blank(K), blank(K), blank(KK), blank(2 * H)
    mu[:, :, :nd] = np.arange(K)[None, :, None] + 0.3 * rng.standard_normal((W, K, nd))
    sig2[:, :, :nd] = 0.2 + rng.gamma(3.0, 0.25, (W, K, nd))
    pi_end[:, :, :nd] = np.moveaxis(rng.dirichlet(np.full(K, 2.0), (W, nd)), 2, 1)
    A[:, :, :nd] = np.moveaxis(rng.dirichlet(np.full(K, 1.5), (W, nd, K)).reshape(W, nd, KK), 2, 1)
    fcast[:, 0, :nd] = 2.0 + 0.5 * mu[:, 0, :nd] + 0.4 * rng.standard_normal((W, nd))
    if kind == "outlier":
        mu[:, 0, 0] = 30.0 * 0.3
        sig2[:, 0, :nd] = 1e4 + 1e-2 * rng.standard_normal((W, nd))
    elif kind == "collinear":
        mu[:, 1, :nd] = 0.5 * mu[:, 0, :nd] + 1e-4 * rng.standard_normal((W, nd))
    elif kind == "duplicate":
        mu[:, 1, :nd] = mu[:, 0, :nd]
    elif kind == "negated":
        mu[:, 1, :nd] = -mu[:, 0, :nd]
    elif kind == "sticky":
        pi_end[:, 0, :nd] = 1.0
        for d in sorted({nd // 3, nd // 2, nd - 1} - {0})[:max(nd - 1, 0)]:
            pi_end[:, 0, d] = 0.99999
    elif kind == "constant":
        sig2[:, 1, :nd] = 0.7 + 1e-7 * rng.standard_normal((W, nd))
    return mu, sig2, pi_end, A, fcast


def accumulation_cases():
    """(K, nd, W, H, pad) of the GPU accumulation cases: every K (every PPT) x every nd edge; W, H and pad dealt round-robin."""
    out = []
    for K in range(2, MAXK + 1):
        for i, nd in enumerate(ND_EDGES):
            k = len(out)
            out.append((K, nd, (1, 3)[k % 2], (1, 3, 8)[k % 3], (0, 5)[(k // 2) % 2]))
    return out


KIND_KS = (3, 5, 6, 8)
KIND_ND = 129


def kind_cases():
    """(kind, K, W, H, nd, pad) of the GPU end-to-end cases: every kind at K = 3, 5, 6, 8, two tiles and one draw."""
    return [(kind, K, 2, (1, 3, 8)[(i + j) % 3], KIND_ND, 5 * ((i + j) % 2)) for i, kind in enumerate(KINDS) for j, K in enumerate(KIND_KS)]


SPLIT_SHAPES = ((3, 200), (5, 200), (8, 200))          # (K, nd) of the block-split cases; kind outlier, W = 2, H = 3
SPLIT_NAMES = ("1+rest", "63+rest", "64+rest", "65+rest", "137s")
SPLIT_ONES = ((3, 65), (6, 65), (7, 3))                # ... and of the runs in blocks of one draw each


def split_cases():
    """(K, nd, name) of the GPU block-split cases."""
    return [(K, nd, name) for K, nd in SPLIT_SHAPES for name in SPLIT_NAMES] + [(K, nd, "ones") for K, nd in SPLIT_ONES]


def split_blocks(nd, name):
    """The draw counts of the consecutive launches of a split: 'H+rest', '137s' (blocks of 137), 'ones'."""
    if name == "ones":
        return [1] * nd
    if name == "137s":
        return [137] * (nd // 137) + ([nd % 137] if nd % 137 else [])
    head = int(name.split("+")[0])
    return [head, nd - head]


def case_seed(K, nd, kind="plain"):
    return 100000 * KINDS.index(kind) + 1000 * K + nd
