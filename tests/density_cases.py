"""Reference, tolerance and cases for the chain-density tests (no GPU): a numpy restatement of the rules of
hmcg_chain_density[_device] in include/hmcg.h that every check compares against.

Counts, range and NaN positions are compared EXACTLY: the bin rule is four rounded fp64 operations (x' - lo, hi - lo, B / that,
the product) and a floor, the same in numpy and on the device; rounding is np.rint(x * 1e5) / 1e5 with the value itself where
that is not finite (csrc/round5.hpp computes the correctly rounded quotient).

Moments and trace are taken in np.longdouble, two-pass: a_d = x'_d - p exactly (p = x' of draw 0, the library's pivot, so a
non-finite draw 0 poisons the reference as it poisons the library), m = sum a / n, mean = p + m, variance =
sum (a - m)^2 / (n - 1); the trace from the running sum of a.

Tolerances, derived from the shape of the library's computation, nothing measured.  u = 2^-53, R = max |x' - p| over the prefix,
n its length.
  mean = p + S1 / n.  a_d = fl(x' - p) errs by at most u R.  n such terms added in ANY fixed order: the sum errs by at most
    n u R (the terms) + (n - 1) u n R (the additions, each partial sum at most n R), so S1 / n by [1 + (n - 1)] u R = n u R;
    the division adds u R, the final addition u |mean|.  That is (n + 1) u R + u |mean|; two more u R cover the second-order
    terms and the longdouble reference's own rounding (2^-64 in place of u).  Bound: (n + 3) u R + u |mean|.
  variance = (S2 - S1^2 / n) / (n - 1).  a^2 carries 3 u (two from a, one product), S2 = sum a^2 <= n R^2 then (n + 2) u n R^2.
    S1^2 / n <= n R^2 carries twice S1's relative n u, a product and a division: (2 n + 2) u n R^2.  The difference and the last
    division two more roundings of at most n R^2.  Sum: (3 n + 6) u n R^2 / (n - 1) <= (3 n + 6) 2 u R^2 for n >= 2.
    Bound: (3 n + 7) 2^-52 R^2, the form of tests/bias_cases.py.  A constant column has R = 0: the bound is 0 and the library
    gives exactly 0.
  trace point i: the mean bound with n_i = (i + 1) stride and R over those draws.
Cells where the reference is +-inf must hold the same infinity; NaN positions must match exactly."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SLAB = 1024
ND = (1, 2, 63, 65, 255, 257, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 17)
EXACT = ("counts", "below", "above", "nan", "range")


def round5(x):
    """The cell rounding of the per-draw files: rint(x * 1e5) / 1e5, the value itself where that is not finite."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.rint(x * 1e5) / 1e5
    return np.where(np.isfinite(q), q, x)


def histogram(v, lo, hi, B):
    """The bin rule on a 1-D array: (slot per value, -1 below, -2 above, -3 nan)."""
    v = np.asarray(v, dtype=np.float64)
    B = int(B)
    isn = np.isnan(v)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        norange = bool(np.isnan(lo) or np.isnan(hi))
        below = ~isn & (np.full(v.shape, norange) | (v < lo))
        above = ~isn & ~below & (v > hi)
        slot = np.zeros(v.shape, dtype=np.int64)
        if hi > lo:
            off = v - np.float64(lo)
            width = np.float64(hi) - np.float64(lo)
            scale = np.float64(B) / width
            t = np.floor(off * scale)
            t = np.where(np.isnan(t), 0.0, t)
            slot = np.clip(t, 0.0, float(B - 1)).astype(np.int64)
    slot[below] = -1
    slot[above] = -2
    slot[isn] = -3
    return slot


def reference(x, cuts=None, bins=64, lo_hi=None, trace=(0, 1), round5_=True, nd=None):
    """x (W, ..., ld), draw index last, every axis between counted as columns; the first nd draws.  Returns the dict of
    _lib.unpack_chain_density (mean / variance / trace as longdouble) plus R (W, C, n_cuts) and trace_R (W, C, trace_len) for
    `tolerance`."""
    x = np.asarray(x, dtype=np.float64)
    W, ld = x.shape[0], x.shape[-1]
    nd = ld if nd is None else int(nd)
    xs = x.reshape(W, -1, ld)[:, :, :nd]
    Cn = xs.shape[1]
    cuts = (nd,) if cuts is None else tuple(int(c) for c in cuts)
    B, nc = int(bins), len(cuts)
    xr = round5(xs) if round5_ else xs.copy()
    fin = np.isfinite(xr)
    if lo_hi is None:
        lo = np.where(fin, xr, np.inf).min(axis=2)
        hi = np.where(fin, xr, -np.inf).max(axis=2)
        none = ~fin.any(axis=2)
        lo[none] = np.nan
        hi[none] = np.nan
    else:
        lo_hi = np.asarray(lo_hi, dtype=np.float64).reshape(W, Cn, 2)
        lo, hi = lo_hi[..., 0].copy(), lo_hi[..., 1].copy()
    out = {"counts": np.zeros((W, Cn, nc, B), dtype=np.int64), "below": np.zeros((W, Cn, nc), dtype=np.int64),
           "above": np.zeros((W, Cn, nc), dtype=np.int64), "nan": np.zeros((W, Cn, nc), dtype=np.int64),
           "range": np.stack([lo, hi], axis=-1)}
    for w in range(W):
        for c in range(Cn):
            slot = histogram(xr[w, c], lo[w, c], hi[w, c], B)
            for j, cut in enumerate(cuts):
                s = slot[:cut]
                out["counts"][w, c, j] = np.bincount(s[s >= 0], minlength=B)
                out["below"][w, c, j], out["above"][w, c, j], out["nan"][w, c, j] = (s == -1).sum(), (s == -2).sum(), (s == -3).sum()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        p = xr[:, :, :1].astype(LD)
        a = xr.astype(LD) - p
        absa = np.abs(a).astype(np.float64)
        mean, var, R = (np.empty((W, Cn, nc), dtype=LD) for _ in range(3))
        for j, cut in enumerate(cuts):
            n = LD(cut)
            m = a[:, :, :cut].sum(axis=2) / n
            mean[:, :, j] = p[:, :, 0] + m
            var[:, :, j] = ((a[:, :, :cut] - m[:, :, None]) ** 2).sum(axis=2) / (n - 1)
            R[:, :, j] = absa[:, :, :cut].max(axis=2)
        tl, ts = int(trace[0]), int(trace[1])
        idx = (np.arange(tl) + 1) * ts - 1
        run = np.cumsum(a, axis=2)
        out["trace"] = p + run[:, :, idx] / (idx + 1).astype(LD)
        out["trace_R"] = np.maximum.accumulate(absa, axis=2)[:, :, idx]
        out["trace_n"] = (idx + 1).astype(np.float64)
    out["mean"], out["variance"], out["R"] = mean, var, R.astype(np.float64)
    out["cuts"] = cuts
    return out


def tolerance(ref):
    """Absolute bounds per cell of mean, variance and trace (module docstring).  Non-finite reference cells give non-finite
    bounds; those cells are compared by position and sign only."""
    n = np.asarray(ref["cuts"], dtype=np.float64)[None, None, :]
    R = ref["R"]
    with np.errstate(invalid="ignore", over="ignore"):
        return {"mean": (n + 3.0) * U * R + U * np.abs(ref["mean"].astype(np.float64)),
                "variance": (3.0 * n + 7.0) * 2.0 * U * R * R,
                "trace": (ref["trace_n"] + 3.0) * U * ref["trace_R"] + U * np.abs(ref["trace"].astype(np.float64))}


def check(got, ref, label=""):
    """got: the dict of _lib.unpack_chain_density.  Counts, below, above, nan and range array_equal (NaN range cells by position);
    the four groups of every prefix sum to its cut; mean, variance and trace within `tolerance`, NaN and inf positions exactly.
    Prints and returns the largest |diff| / bound per float output."""
    for key in EXACT:
        g, r = np.asarray(got[key]), ref[key]
        assert g.shape == r.shape, (label, key, g.shape, r.shape)
        assert np.array_equal(g, r, equal_nan=(key == "range")), (label, key, g, r)
    total = got["counts"].sum(axis=3) + got["below"] + got["above"] + got["nan"]
    assert np.array_equal(total, np.broadcast_to(np.asarray(ref["cuts"], dtype=np.int64), total.shape)), (label, "groups do not sum to the cuts")
    tol = tolerance(ref)
    worst = {}
    for key in ("mean", "variance", "trace"):
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
    return worst


EDGE_LO, EDGE_HI = -1.0, 1.0        # the range the bin-edge column is built for


def make_case(seed, W, Cn, nd, pad=0, bins=64):
    """(W, Cn, nd + pad) draws, NaN in the padding (a counted NaN then proves the padding was read).  Column c plays the part
    c % 8: 0, 7 draws clustered the way posteriors are (a narrow normal about a centre, a second mode now and then); 1 values
    exactly on the bin edges EDGE_LO + j (EDGE_HI - EDGE_LO) / bins, both ends included; 2 a handful of values many times over,
    -0.0 and 0.0 among them; 3 a constant; 4 clustered with NaN, +inf and -inf sprinkled in (window 2 has +inf at draw 0, the
    pivot); 5 no finite value; 6 an offset of 1e4 with a spread of 1e-2."""
    rng = np.random.default_rng(seed)
    x = np.full((W, Cn, nd + pad), np.nan)
    for w in range(W):
        for c in range(Cn):
            part = c % 8
            centre = rng.normal(3.0, 2.0)
            v = centre + 0.3 * rng.standard_normal(nd)
            far = rng.random(nd) < 0.1
            v[far] += 1.5
            if part == 1:
                v = EDGE_LO + rng.integers(0, bins + 1, size=nd) * (EDGE_HI - EDGE_LO) / bins
                v[rng.integers(0, nd)] = EDGE_LO
                v[rng.integers(0, nd)] = EDGE_HI
            elif part == 2:
                v = rng.choice(np.array([0.0, -0.0, 1.5, -2.25, 1.5000049, 1.5000051]), size=nd)
            elif part == 3:
                v = np.full(nd, 7.125)
            elif part == 4:
                for bad in (np.nan, np.inf, -np.inf):
                    v[rng.integers(min(1, nd - 1), nd, size=max(1, nd // 40))] = bad
                if w == 2:
                    v[0] = np.inf
            elif part == 5:
                v = rng.choice(np.array([np.nan, np.inf, -np.inf]), size=nd)
            elif part == 6:
                v = 1e4 + 1e-2 * rng.standard_normal(nd)
            x[w, c, :nd] = v
    return x


def cut_set(kind, nd):
    """The cut sets the tests deal round-robin: 0 the whole chain, 1 (1, nd), 2 a slab boundary (and nd), 3 two cuts inside the
    last slab (and nd), 4 eight cuts.  Always strictly ascending within 1..nd."""
    if kind == 0:
        c = [nd]
    elif kind == 1:
        c = [1, nd]
    elif kind == 2:
        c = [SLAB, nd] if nd > SLAB else [max(1, nd // 2), nd]
    elif kind == 3:
        s0 = (nd - 1) // SLAB * SLAB
        c = [s0 + max(1, (nd - s0) // 3), s0 + max(1, 2 * (nd - s0) // 3), nd]
    else:
        c = [int(v) for v in np.linspace(1, nd, 8)]
    return tuple(sorted(set(v for v in c if 1 <= v <= nd)))


def trace_set(kind, nd):
    """0 no trace, 1 stride 1 over everything, 2 stride 7 ending inside a slab."""
    if kind == 0:
        return (0, 1)
    if kind == 1:
        return (nd, 1)
    return (max(nd - 3, 0) // 7, 7)


def given_range(kind, ref_auto, W, Cn):
    """0 automatic (None); 1 narrower than the data: the middle half of the automatic range (EDGE_LO, EDGE_HI for the bin-edge
    columns, so that values sit exactly on the edges; 0, 1 where there is no finite value); 2 hi == lo at the automatic lo."""
    if kind == 0:
        return None
    r = ref_auto["range"]
    lo = np.where(np.isnan(r[..., 0]), 0.0, r[..., 0])
    hi = np.where(np.isnan(r[..., 1]), 1.0, r[..., 1])
    if kind == 2:
        return np.stack([lo, lo], axis=-1)
    a, b = lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo)
    edge = (np.arange(Cn) % 8 == 1)[None, :] & np.ones((W, 1), dtype=bool)
    a, b = np.where(edge, EDGE_LO, a), np.where(edge, EDGE_HI, b)
    return np.stack([a, b], axis=-1)
