"""Case table of tests/test_gpu_config_range.py, and what tests/test_config_range_cases.py holds it to without a GPU.

The rest of the GPU suite moves along the time axis (T, K, kernel form).  These cases move along the width of the per-draw
output block and across the range of hmcg_config's scalar fields, at the smallest shape that reaches each mechanism:
  * H = 0..8 horizons (HMCG_MAXH) on the register-resident and the LDS-resident kernel, H = 8 on every route: the forecast
    lanes, sh.fcval, the strides NS = 3K + K^2 + 2H of summary / sample_summary and NS + K of sumacc, the 2H-wide chunk
    columns and scatter of the host entries;
  * every blend_mask bit 0..7, with a junk horizon in blended slots (include/hmcg.h: ignored);
  * horizons 25 | 26 | 27 together (the register-resident kernel changes its forecast route beyond 26), a repeated horizon,
    0, 1 and 5000; never beyond 5000: two evaluation orders of A^h drift apart by about h K eps, and 5000 * 8 * 1.1e-16
    stays four orders under the suite's 1e-9;
  * 64-bit seeds (a non-zero upper Philox key word), window ids with the top bit set, window_base + w wrapping past 2^32;
  * priors other than the two the suite uses (alpha = 3.5, nu = 0.25 on the base path);
  * a yreal row with one unknown (NaN) cell, a different column in every H = 8 case.

A case is a Case tuple; inputs() builds its data, gpu_call() and oracle_window() the two sides' arguments from the same
fields, so that the CPU contract and the GPU test cannot drift apart."""
import collections

import numpy as np

from hmc_jl_amd import synth

import kernel_tables as kt
from kernel_tables import NT

FULL = (0, 1, 25, 26, 27, 12, 12, 5000)              # H = 4..7 use its prefixes
REVERSED = (5000, 0, 27, 26)                         # lane order ascending, horizon order not
JUNK_HORIZON = 999999                                # in a blended slot: ignored
MAX_HORIZON = 5000
SEED_DEFAULT = 1234
SEED_GOLDEN = 0x9E3779B97F4A7C15
SEED_HIGH_WORD = 1234 + 2 ** 32                      # the suite's default in the low word
TOP_IDS = (0x80000000, 0xFFFFFFFF, 0)
WRAP_BASE = 0xFFFFFFFE                               # ids 0xFFFFFFFE, 0xFFFFFFFF, 0 at W = 3
SWEEPS, SPLIT_SWEEPS = (1, 3), (2, 5)
# extras.corr is a matrix of Pearson correlations: over three draws nearly every entry is within rounding of +-1 and a
# column that happens to be constant after rounding is NaN, so that run alone keeps more draws (two GPU runs, no oracle)
CORR_SWEEPS = (2, 40)
N_SAMPLES = 3
KAPPA, TAIL_SIGMA = 0.6, (0.4, 1.3, 0.05)
ROUTES = ("register", "tpw", "lds", "stream")        # what the dispatch must pick; "tpw": a register-resident row with a thread count of its own
PATHS = ("base", "sig", "tail")

Case = collections.namedtuple("Case", "id route path K lens sweeps horizons blend seed window_ids window_base alpha nu nan_col env tpw sigLen split")
# lens: window lengths; sweeps: (burnin, nrun); blend: the blend_mask bits (tail path); window_ids: explicit ids or None (then
# window_base + w); nan_col: the yreal column that is unknown (None: all known); env: the diagnostic switches the case sets;
# tpw: threads_per_window (0: auto); sigLen: signal steps past the end date (tail path); split: the chain is also cut and resumed


def _case(id, route, path, K, lens, horizons, blend=(), seed=SEED_DEFAULT, window_ids=None, window_base=0, alpha=None, nu=None,
          env=(), tpw=0, sigLen=0, sweeps=SWEEPS, split=False):
    prior = 1.0 if path == "base" else 2.0           # HyperParams(Y, D) on the base path, HyperParams(opt) on the signal paths
    if window_ids is not None:
        window_ids = tuple(window_ids[:len(lens)])
    return Case(id, route, path, K, tuple(lens), sweeps, tuple(horizons), tuple(blend), seed, window_ids, window_base,
                prior if alpha is None else alpha, prior if nu is None else nu, None, tuple(env), tpw, sigLen, split)


def _blended(horizons, bits, junk):
    return tuple(JUNK_HORIZON if junk and k in bits else h for k, h in enumerate(horizons))


def _tail(id, route, K, T, sigLen, bits, junk, **kw):
    return _case(id, route, "tail", K, (T, T - 7, T - 64), _blended(FULL, bits, junk), blend=bits, sigLen=sigLen, **kw)


REG_LENS = (200, 65, 2)                              # one steps-per-thread class (L = 1), a wave boundary, the shortest window


def FLV(flavour):
    return (("HMCG_FLAVOUR", flavour),)


FORCE_BIG, FORCE_STREAM = (("HMCG_FORCE_BIG", "1"),), (("HMCG_FORCE_STREAM", "1"),)

_TABLE = [
    # register-resident, K = 2..4 in each flavour: `h` has OUT_WAVE / FC_WAVE on helper waves, p1 / p2 on waves 1 and NW - 1
    _case("reg-K2-p1-H8", "register", "base", 2, REG_LENS, FULL, env=FLV("p1"), seed=SEED_GOLDEN),
    _case("reg-K2-p2-H4", "register", "base", 2, REG_LENS, FULL[:4], env=FLV("p2"), window_ids=TOP_IDS),
    _case("reg-K2-h-H5", "register", "base", 2, REG_LENS, FULL[:5], env=FLV("h"), window_base=WRAP_BASE),
    _case("reg-K3-p1-H6", "register", "base", 3, REG_LENS, FULL[:6], env=FLV("p1"), seed=SEED_HIGH_WORD),
    _case("reg-K3-p2-H7", "register", "base", 3, REG_LENS, FULL[:7], env=FLV("p2"), alpha=3.5, nu=0.25),
    _case("reg-K3-h-H8", "register", "base", 3, REG_LENS, FULL, env=FLV("h"), window_base=WRAP_BASE, seed=SEED_HIGH_WORD),
    _case("reg-K4-p1-H4r", "register", "base", 4, REG_LENS, REVERSED, env=FLV("p1"), seed=SEED_GOLDEN),
    _case("reg-K4-p2-H8", "register", "base", 4, REG_LENS, FULL, env=FLV("p2"), window_ids=TOP_IDS, seed=SEED_GOLDEN),
    _case("reg-K4-h-H3", "register", "base", 4, REG_LENS, FULL[:3], env=FLV("h")),
    _case("reg-K3-H0", "register", "base", 3, REG_LENS, ()),
    _case("reg-K3-H1", "register", "base", 3, REG_LENS, FULL[:1]),
    _case("reg-K3-H2", "register", "base", 3, REG_LENS, FULL[:2]),
    # the two rows with a thread count of their own, at their own shape: (3, 8, 128) has parameter and forecast lanes in one wave
    _case("tpw-K3-L8-NT128-H8", "tpw", "base", 3, (1000, 1000, 1000), FULL, tpw=128, seed=SEED_GOLDEN, window_ids=TOP_IDS),
    _case("tpw-K3-L2-NT512-H8", "tpw", "base", 3, (1000, 1000, 1000), FULL, tpw=512, seed=SEED_HIGH_WORD, window_base=WRAP_BASE),
    # LDS-resident: K = 7 has 70 parameter outputs (a second output pass), K = 3 by the diagnostic switch
    _case("lds-K5-H6", "lds", "base", 5, (130, 64, 2), FULL[:6], window_base=WRAP_BASE),
    _case("lds-K7-H7", "lds", "base", 7, (130,), FULL[:7], seed=SEED_HIGH_WORD),
    _case("lds-K8-H8", "lds", "base", 8, (300, 65), FULL, seed=SEED_GOLDEN, window_ids=TOP_IDS),
    _case("lds-K3-forced-H5", "lds", "base", 3, (200,), FULL[:5], env=FORCE_BIG, alpha=3.5, nu=0.25),
    _case("lds-K6-H4r", "lds", "base", 6, (130,), REVERSED, window_ids=TOP_IDS[1:]),
    _case("lds-K5-H0", "lds", "base", 5, (130,), ()),
    _case("lds-K5-H1", "lds", "base", 5, (130,), FULL[:1]),
    _case("lds-K5-H2", "lds", "base", 5, (130,), FULL[:2]),
    _case("lds-K5-H3", "lds", "base", 5, (130,), FULL[:3]),
    _case("lds-K6-H4", "lds", "base", 6, (130,), FULL[:4]),
    _case("lds-K5-H8", "lds", "base", 5, (130, 64, 2), FULL, window_base=WRAP_BASE, seed=SEED_HIGH_WORD),
    # streaming form of the LDS-resident kernel
    _case("stream-K3-H8", "stream", "base", 3, (300,), FULL, env=FORCE_BIG + FORCE_STREAM, seed=SEED_GOLDEN, window_ids=TOP_IDS),
    _case("stream-K8-H8", "stream", "base", 8, (300, 257, 2), FULL, env=FORCE_STREAM, seed=SEED_HIGH_WORD, window_base=WRAP_BASE),
    # signal path: three chained noise samples, sample_summary
    _case("reg-sig-K3-H8", "register", "sig", 3, (140, 133), FULL, seed=SEED_GOLDEN, window_ids=TOP_IDS),
    _case("lds-sig-K6-H8", "lds", "sig", 6, (150,), FULL, seed=SEED_HIGH_WORD, window_ids=TOP_IDS[1:]),
    # signals past the end date: one blend bit in the middle of the block; two bits with a junk horizon in their slots
    _tail("reg-tail-K3-bit5", "register", 3, 140, 12, (5,), False),
    _tail("reg-tail-K3-bits37-junk", "register", 3, 140, 12, (3, 7), True, seed=SEED_GOLDEN),
    _tail("reg-tail-K3-bits0246-junk", "register", 3, 140, 12, (0, 2, 4, 6), True, window_ids=(0xFFFFFFFE, 0xFFFFFFFF, 0)),
    _tail("lds-tail-K8-bit5", "lds", 8, 200, 48, (5,), False, window_ids=TOP_IDS),
    _tail("lds-tail-K8-bits37-junk", "lds", 8, 200, 48, (3, 7), True, seed=SEED_HIGH_WORD),
    _tail("lds-tail-K8-bit1-junk", "lds", 8, 200, 48, (1,), True),
    # H = 8 chains that are also cut and resumed (two burn-in sweeps, so that a cut can fall inside burn-in)
    _case("split-reg-K3-H8", "register", "base", 3, REG_LENS, FULL, sweeps=SPLIT_SWEEPS, split=True, seed=SEED_GOLDEN),
    _case("split-lds-K5-H8", "lds", "base", 5, (130, 64, 2), FULL, sweeps=SPLIT_SWEEPS, split=True, window_ids=TOP_IDS),
    _case("split-sig-K3-H8", "register", "sig", 3, (140, 133), FULL, sweeps=SPLIT_SWEEPS, split=True, seed=SEED_HIGH_WORD),
]


def _with_unknown_columns(table):
    """One yreal column unknown in every H = 8 case, a different one from case to case."""
    out, n = [], 0
    for c in table:
        if len(c.horizons) == 8:
            c = c._replace(nan_col=(3 * n + 1) % 8)       # 1, 4, 7, 2, 5, 0, 3, 6, ...
            n += 1
        out.append(c)
    return out


CASES = _with_unknown_columns(_TABLE)
BY_ID = {c.id: c for c in CASES}
# cuts of a split chain, in sweeps: inside burn-in, at burnin, after a kept draw (on the signal path: of the first noise sample)
SPLIT_CUTS = ((1,), (2,), (4,))


# ---------------------------------------------------------------- data -------
def is_sig(c):
    return c.path in ("sig", "tail")


def ids_of(c):
    """The RNG stream id of every window, as the library numbers them."""
    if c.window_ids is not None:
        return [int(i) for i in c.window_ids]
    return [(c.window_base + w) & 0xFFFFFFFF for w in range(len(c.lens))]


def inputs(c):
    """Y (W, ldY), Tw (W,), yreal (W, H): the realised values are the window's next H points, one column unknown."""
    W, H = len(c.lens), len(c.horizons)
    Y, Tw, fut = synth.generate_panel(W, max(c.lens), c.K, ragged=list(c.lens))
    yreal = np.ascontiguousarray(fut[:, :H])
    if c.nan_col is not None:
        yreal[:, c.nan_col] = np.nan
    return Y, Tw, yreal


def signal_inputs(c, Tw):
    """sig_range, save_range, sigma_signal, end_pos (None on the plain signal path) of a signal-path case."""
    W = len(Tw)
    if c.path == "tail":
        sig = np.stack([Tw - c.sigLen, Tw], axis=1).astype(np.int32)
        return sig, sig.copy(), np.array(TAIL_SIGMA[:W]), (Tw - 1 - c.sigLen).astype(np.int32)
    sig = np.stack([Tw - np.array([40, 1, 25][:W]), Tw], axis=1).astype(np.int32)        # a tail, one step
    save = np.stack([Tw - 2, Tw], axis=1).astype(np.int32)
    return sig, save, np.array([0.5, 1.0, 0.2][:W]), None


def blend_mask(c):
    return sum(1 << b for b in c.blend)


def gpu_call(c, **over):
    """(args, kw) of _lib.estimate_batch_host / device_entry.estimate_batch_device_np for the case.  over: fields replaced or
    added (None removes one)."""
    Y, Tw, yreal = inputs(c)
    burnin, nrun = over.pop("sweeps", c.sweeps)
    horizons = over.pop("horizons", c.horizons)
    if len(horizons) != len(c.horizons):
        yreal = np.ascontiguousarray(yreal[:, :len(horizons)])
    kw = dict(want_state=True, seed=c.seed)
    if c.window_ids is not None:
        kw["window_ids"] = np.array(c.window_ids, dtype=np.uint32)
    if c.window_base:
        kw["window_base"] = c.window_base
    if c.tpw:
        kw["threads_per_window"] = c.tpw
    if is_sig(c):
        sig, save, ssig, end_pos = signal_inputs(c, Tw)
        kw.update(sig_range=sig, save_range=save, sigma_signal=ssig, kappa=KAPPA, n_samples=N_SAMPLES, alpha=c.alpha, nu=c.nu,
                  want_sample_summary=True)
        if c.path == "tail":
            kw.update(end_pos=end_pos, blend_mask=blend_mask(c))
    elif (c.alpha, c.nu) != (1.0, 1.0):
        kw.update(alpha=c.alpha, nu=c.nu)
    kw.update(over)
    kw = {k: v for k, v in kw.items() if v is not None}
    return (Y, Tw, c.K, burnin, nrun, horizons, yreal), kw


def oracle_window(oracle, c, w, Y, Tw, yreal, horizons=None):
    """The oracle's run of window w of the case (horizons: instead of the case's own)."""
    hz = c.horizons if horizons is None else tuple(horizons)
    burnin, nrun = c.sweeps
    kw = dict(alpha=c.alpha, nu=c.nu, horizons=hz, yreal=yreal[w], seed=c.seed, window_id=ids_of(c)[w])
    n_samples = 1
    if is_sig(c):
        sig, save, ssig, end_pos = signal_inputs(c, Tw)
        n_samples = N_SAMPLES
        kw.update(sig=tuple(int(v) for v in sig[w]), save=tuple(int(v) for v in save[w]), kappa=KAPPA, sigma_signal=float(ssig[w]))
        if c.path == "tail":
            kw.update(end_pos=int(end_pos[w]), blend_mask=blend_mask(c))
    return oracle.estimate_signals(Y[w, :Tw[w]], c.K, burnin, nrun, n_samples, **kw)


# ------------------------------------------------- the high-precision check --
def forecast_longdouble(pi_end, A, mu, h):
    """pi_end[d]' A[d]^h mu[d] for every draw d in numpy.longdouble, by square-and-multiply: pi_end, mu (nd, K), A (nd, K, K)
    with A[d, i, j] = P(j | i).  The value does not depend on the label order, as long as the three share it."""
    M = np.asarray(A, dtype=np.longdouble)
    v = np.asarray(mu, dtype=np.longdouble)[:, :, None]
    h = int(h)
    while h:
        if h & 1:
            v = np.matmul(M, v)
        h >>= 1
        if h:
            M = np.matmul(M, M)
    return np.einsum("dk,dk->d", np.asarray(pi_end, dtype=np.longdouble), v[:, :, 0])


def forecast_distance(fcast, pi_end, A, mu, horizons, skip=()):
    """Largest distance, relative to 1 + |x|, between the forecast columns fcast[:, 2k] (nd, 2H) and the recomputation from the
    same run's draws, over the slots not in `skip`."""
    worst = 0.0
    for k, h in enumerate(horizons):
        if k in skip:
            continue
        ref = forecast_longdouble(pi_end, A, mu, h)
        got = np.asarray(fcast[:, 2 * k], dtype=np.longdouble)
        worst = max(worst, float(np.max(np.abs(got - ref) / (1.0 + np.abs(ref)))))
    return worst


def rounded_means(mu, sig2, pi_end, A, fcast):
    """runaggregate's row of one window from its draws in the C-ABI layouts (draw index last; A (K, K, nd) column-major):
    mean over draws of round(x, 5), rows mu | sig2 | pi_end | A(:) | fcast."""
    nd = mu.shape[-1]
    rows = np.concatenate([mu, sig2, pi_end, A.reshape(-1, nd), fcast], axis=0)
    return (np.rint(rows * 1e5) / 1e5).mean(axis=1)


# ------------------------------------------------------ route of a case ------
def planned_route(c):
    """What the planner does with the case's lengths and switches, from the parsed variant tables (no GPU): the route, and on
    the register-resident routes the steps per thread."""
    env = dict(c.env)
    sig, top = is_sig(c), max(c.lens)
    if c.tpw:
        mine = [(K, L, nt) for (K, L, nt) in kt.OWN_THREAD_COUNT if (K, nt) == (c.K, c.tpw) and nt * L >= top > nt * L // 2]
        return ("tpw", mine[0][1]) if mine and not env else ("none", 0)
    if "HMCG_FORCE_BIG" not in env and top <= kt.ladder_ceiling(c.K, sig, False):
        return ("none", 0) if "HMCG_FORCE_STREAM" in env else ("register", kt.steps_per_thread(c.K, top, sig))
    L = (top + NT - 1) // NT
    stream = "HMCG_FORCE_STREAM" in env or kt.dyn_bytes(L) > kt.LDS_LIMIT
    return ("stream" if stream else "lds"), L
