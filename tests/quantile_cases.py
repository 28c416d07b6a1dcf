"""Reference and cases for the exact-quantile tests (no GPU): a numpy restatement of the rules of hmcg_chain_quantiles[_device]
in include/hmcg_order.h that every check compares against, BIT FOR BIT: the result of a selection is an element of its input,
so nothing here has a tolerance.

x' = round5(x) (np.rint(x * 1e5) / 1e5, the value itself where that is not finite: density_cases.round5) or x.  NaNs are split
off and counted.  The rest is sorted, stably, on the order-preserving integer key u = bits(x'); key = (u >> 63) ? ~u : u | 2^63,
so that -0.0 stands below +0.0 as in the IEEE total order.  Per probability the rank rule is restated one rounded fp64
operation at a time: h = p * (m - 1), j = floor(h), g = h - j, lo = x_(j), hi = x_(min(j + 1, m - 1)); `restate` is the value
rule: lo when g == 0 or lo == hi, else v = lo + g * (hi - lo) clamped to hi."""
import numpy as np

from density_cases import round5

FIELDS = ("value", "lo", "hi", "g")
TOP = np.uint64(1) << np.uint64(63)
ND_EDGES = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4097, 50003)     # a wave, a tile of 4096 draws, the 4096 candidates of LDS
PROBS3 = (0.05, 0.5, 0.95)
# 0, 1, the median, a duplicate, unsorted, and p = k / 4, k / 8: h = p (m - 1) is an exact integer whenever 8 divides m - 1
PROBS16 = (0.5, 0.0, 1.0, 0.95, 0.05, 0.25, 0.75, 0.5, 0.125, 0.875, 0.025, 0.975, 1.0 / 3.0, 0.999999, 1e-6, 0.625)
M_EDGES = (1, 2, 3, 4, 5, 9, 64, 65, 1025, 4097, 50003, 250000, 2 ** 31 - 1)
P_EDGES = (0.0, 1.0, 0.5, 0.25, 0.05, 0.95, 1.0 / 3.0, 1e-6, 0.999999, 0.125, 1.0 - 2.0 ** -53)


def key_of(x):
    """The order-preserving uint64 key of an array of doubles."""
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | TOP)


def unkey(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where(k >> np.uint64(63) != 0, k & ~TOP, ~k).view(np.float64)


def rank(p, m):
    """(j, g) of probability p among m ranked values."""
    h = np.float64(p) * np.float64(m - 1)
    j = int(np.floor(h))
    return j, h - np.float64(j)


def restate(lo, hi, g):
    """`value` from lo, hi and g, elementwise, by the ABI's rule."""
    lo, hi, g = (np.asarray(a, dtype=np.float64) for a in (lo, hi, g))
    with np.errstate(invalid="ignore", over="ignore"):
        diff = hi - lo
        step = g * diff
        v = lo + step
        v = np.where(v > hi, hi, v)
        return np.where((g == 0.0) | (lo == hi), lo, v)


def reference(x, probs, round5_=True, nd=None):
    """x (W, ..., ld), draw index last, every axis between counted as columns; the first nd draws.  Returns the dict of
    _lib.unpack_chain_quantiles."""
    x = np.asarray(x, dtype=np.float64)
    W, ld = x.shape[0], x.shape[-1]
    nd = ld if nd is None else int(nd)
    xs = x.reshape(W, -1, ld)[:, :, :nd]
    Cn, Q = xs.shape[1], len(probs)
    xr = round5(xs) if round5_ else xs.copy()
    out = {k: np.full((W, Cn, Q), np.nan) for k in FIELDS}
    out["count"], out["nan"] = np.zeros((W, Cn), dtype=np.int64), np.zeros((W, Cn), dtype=np.int64)
    for w in range(W):
        for c in range(Cn):
            v = xr[w, c]
            v = v[~np.isnan(v)]
            m = v.size
            out["count"][w, c], out["nan"][w, c] = m, nd - m
            if m == 0:
                continue
            s = unkey(np.sort(key_of(v), kind="stable"))
            for i, p in enumerate(probs):
                j, g = rank(p, m)
                out["lo"][w, c, i], out["hi"][w, c, i], out["g"][w, c, i] = s[j], s[min(j + 1, m - 1)], g
    out["value"] = restate(out["lo"], out["hi"], out["g"])
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def check(got, ref, label=""):
    """lo, hi, g, count, nan bit for bit against the reference; value bit for bit against `restate` of the device's own lo, hi
    and g; NaN positions separately."""
    for key in ("count", "nan"):
        assert got[key].dtype == np.int64 and np.array_equal(got[key], ref[key]), (label, key, got[key], ref[key])
    for key in ("lo", "hi", "g"):
        g, r = np.asarray(got[key]), np.asarray(ref[key])
        assert g.shape == r.shape, (label, key, g.shape, r.shape)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (label, key, "NaN positions")
        ok = ~np.isnan(r)
        assert np.array_equal(bits(g)[ok], bits(r)[ok]), (label, key, g[ok][bits(g)[ok] != bits(r)[ok]][:4], r[ok][bits(g)[ok] != bits(r)[ok]][:4])
    want = restate(got["lo"], got["hi"], got["g"])
    v = np.asarray(got["value"])
    assert np.array_equal(np.isnan(v), np.isnan(want)), (label, "value", "NaN positions")
    ok = ~np.isnan(want)
    assert np.array_equal(bits(v)[ok], bits(want)[ok]), (label, "value")


def column_kinds(rng, nd):
    """Nine differently distributed columns of nd draws: a wrong block index shows."""
    n = rng.standard_normal
    return [1.5 + 0.1 * n(nd), np.exp(n(nd)), -3.0 + 2.0 * n(nd), rng.random(nd), np.where(rng.random(nd) < 0.9, 1.0, rng.random(nd)),
            1e-3 * n(nd), 100.0 + n(nd), np.round(n(nd), 1), -np.exp(2.0 * n(nd))]


def panel(seed, W, Cn, nd, pad=0):
    """(W, Cn, nd + pad) draws, column (w, c) of kind (c + 3 w) mod 9 shifted by w; the padding alternates NaN, -inf, 1e300 so a
    read past nd changes a result."""
    rng = np.random.default_rng(seed)
    x = np.empty((W, Cn, nd + pad))
    fill = np.array([np.nan, -np.inf, 1e300])
    for w in range(W):
        kinds = column_kinds(rng, nd)
        for c in range(Cn):
            x[w, c, :nd] = kinds[(c + 3 * w) % 9] + 0.25 * w
            x[w, c, nd:] = fill[np.arange(pad) % 3]
    return x


# The clamp.  A rounding alone never lifts lo + g * (hi - lo) above hi: d = fl(hi - lo) <= (hi - lo) + ulp(d) / 2, and with
# g <= 1 - 2^-53 the product g * d lies at or below the midpoint under d, so fl(g * d) <= pred(d) <= d - ulp(d) / 2, the exact
# sum lo + fl(g * d) is <= hi and so is its rounding (a search over 10^6 random pairs with `restate` found none either).  What
# does exceed hi is an overflow of hi - lo: for this pair d = inf, v = lo + inf = inf > hi, and the rule gives hi.
CLAMP_LO, CLAMP_HI, CLAMP_P = -1.7976931348623157e308, 1e308, 0.25
