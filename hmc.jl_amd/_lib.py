"""ctypes binding of libhmcgibbs.so (C ABI: include/hmcg.h).

The library is the product: hand-written HIP kernels for gfx950.  There is no
CPU fallback anywhere in this package -- if the shared object is missing or no
GPU is usable, the compute entry points raise.
"""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SO_PATH = os.path.join(CSRC, os.environ.get("HMCG_LIB", "libhmcgibbs.so"))   # HMCG_LIB: diagnostic builds only

HMCG_MAXH = 8
HMCG_MAXK = 8
FLAG_RESUME = 1

ST_BAD_INVGAMMA, ST_EMIS_UNDERFLOW, ST_NONFINITE, ST_GAMMA_CAP, ST_BAD_T, ST_BAD_RANGE = 1, 2, 4, 8, 16, 32
ST_SKIPPED = ST_NONFINITE | ST_BAD_T | ST_BAD_RANGE      # the window was not computed at all

HMCG_MAXTAIL = 256
HMCG_MAXDEV = 16
PRED_ROUND5 = 1
HMCG_MAXGRID = 4096
HMCG_PRED_MAXH = 1024           # largest horizon of the predictive CDFs
PRED_SLAB = 1024                # draws per reduction slab (csrc/stat_plan.hpp): the host entry uploads whole slabs
BIAS_ROUND5 = 1
MIX_ROUND5 = 1
MIX_STRIDE = 8                  # HMCG_MIX_STRIDE: doubles per (window, horizon) of the mixture-moment output
MIX_FIELDS = ("mean", "variance", "skewness", "kurtosis", "within", "between", "draw_skewness", "weight")
DENS_ROUND5 = 1
DENS_MAXBINS = 512              # HMCG_DENS_MAXBINS
DENS_MAXTRACE = 65536           # HMCG_DENS_MAXTRACE
DENS_FIELDS = ("counts", "below", "above", "nan", "range", "mean", "variance", "trace")
ACF_ROUND5 = 1
ACF_MAXLAG = 1024               # HMCG_ACF_MAXLAG
ACF_STRIDE = 8                  # HMCG_ACF_STRIDE: doubles per (window, column) of the diagnostics block
ACF_FIELDS = ("mean", "variance", "tau", "ess", "mcse", "pairs", "truncated", "rhat")
ORD_ROUND5 = 1                  # include/hmcg_order.h
ORD_MAXQ = 16                   # HMCG_ORD_MAXQ: probabilities of one call
ORD_STRIDE = 4                  # HMCG_ORD_STRIDE: doubles per (window, column, probability)
ORD_FIELDS = ("value", "lo", "hi", "g")
ERG_ROUND5 = 1                  # include/hmcg_ergodic.h
FAN_ROUND5 = 1                  # include/hmcg_fan.h
FAN_MAXP = 16                   # HMCG_FAN_MAXP: probabilities of one call
FAN_MAXROUNDS = 10              # HMCG_FAN_MAXROUNDS
FAN_ROUNDS_DEFAULT = 4          # what rounds = 0 means
FAN_STRIDE = 5                  # HMCG_FAN_STRIDE: doubles per (window, horizon, probability)
FAN_FIELDS = ("quantile", "lo", "hi", "Flo", "Fhi")
FAN_NAN, FAN_UNREACHED, FAN_FLAT = 1, 2, 4
SCORE_ROUND5 = 1                # include/hmcg_score.h
SCORE_DRAWS_DEFAULT = 4096      # HMCG_SCORE_DRAWS_DEFAULT: used draws the default thinning leaves at most
SCORE_STRIDE = 5                # HMCG_SCORE_STRIDE: doubles per (window, horizon)
SCORE_FIELDS = ("crps", "e_abs", "e_pair", "pit", "pdf")


def erg_cols(K):
    """HMCG_ERG_COLS(K): per-draw columns of the ergodic moments (pi[K], dur[K], mean, variance)."""
    return 2 * K + 2


def bias_stride(K):
    """HMCG_BIAS_STRIDE(K): doubles per window of the bias-moment output (uncbias, totalbias, mean[2K], cov[2K][2K])."""
    return 2 + 2 * K + 4 * K * K


class HmcgError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("W", C.c_int32), ("K", C.c_int32), ("ldY", C.c_int32),
                ("max_T", C.c_int32), ("burnin", C.c_int32), ("nrun", C.c_int32), ("H", C.c_int32),
                ("horizons", C.c_int32 * HMCG_MAXH), ("seed", C.c_uint64), ("window_base", C.c_uint32),
                ("device", C.c_int32), ("flags", C.c_int32), ("threads_per_window", C.c_int32),
                ("sweep_base", C.c_int32), ("sweep_count", C.c_int32), ("alpha", C.c_double), ("nu", C.c_double),
                ("kappa", C.c_double), ("n_samples", C.c_int32), ("blend_mask", C.c_int32),
                ("min_T", C.c_int32), ("reserved3", C.c_int32)]


class Extras(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("x_init", C.c_void_p),
                ("x_final", C.c_void_p), ("pif_final", C.c_void_p), ("xstate", C.c_void_p), ("sumacc", C.c_void_p), ("window_ids", C.c_void_p),
                ("sig_range", C.c_void_p), ("save_range", C.c_void_p), ("sigma_signal", C.c_void_p),
                ("sigvals", C.c_void_p), ("nsave_ld", C.c_int32), ("reserved2", C.c_int32),
                ("end_pos", C.c_void_p), ("pi_smooth_mean", C.c_void_p), ("pi_filter_mean", C.c_void_p),
                ("corr", C.c_void_p), ("pi_smooth_draws", C.c_void_p), ("sample_summary", C.c_void_p)]


class Timing(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("launches", C.c_int32), ("threads_per_window", C.c_int32),
                ("steps_per_thread", C.c_int32), ("lds_bytes", C.c_int32), ("helper_waves", C.c_int32),
                ("device", C.c_int32), ("call_ms", C.c_double), ("windows", C.c_int32), ("occupancy", C.c_int32),
                ("buckets", C.c_int32), ("streaming", C.c_int32)]


class Predictive(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("W", C.c_int32), ("K", C.c_int32), ("device", C.c_int32),
                ("nd", C.c_int64), ("nd_ld", C.c_int64), ("G", C.c_int32), ("n_h", C.c_int32),
                ("horizons", C.c_int32 * HMCG_MAXH), ("flags", C.c_int32), ("reserved", C.c_int32)]


class Bias(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("W", C.c_int32), ("K", C.c_int32), ("device", C.c_int32),
                ("nd", C.c_int64), ("nd_ld", C.c_int64), ("horizon", C.c_int32), ("H", C.c_int32),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


class Density(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("device", C.c_int32),
                ("nd", C.c_int64), ("nd_ld", C.c_int64), ("B", C.c_int32), ("n_cuts", C.c_int32),
                ("cuts", C.c_int64 * HMCG_MAXH), ("trace_len", C.c_int32), ("flags", C.c_int32), ("trace_stride", C.c_int64)]


class Autocorr(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("device", C.c_int32),
                ("nd", C.c_int64), ("nd_ld", C.c_int64), ("L", C.c_int32), ("flags", C.c_int32)]


class MixMom(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("W", C.c_int32), ("K", C.c_int32), ("device", C.c_int32),
                ("nd", C.c_int64), ("nd_ld", C.c_int64), ("n_h", C.c_int32), ("flags", C.c_int32),
                ("horizons", C.c_int32 * HMCG_MAXH)]


# The five draw statistics: the struct of a call, the stem of its two entries (hmcg_<stem>, hmcg_<stem>_device) and the ROUND5
# bit of its flags.
Stat = collections.namedtuple("Stat", "struct stem round5")
STATS = {"predictive": Stat(Predictive, "predictive_cdf", PRED_ROUND5), "bias": Stat(Bias, "bias_moments", BIAS_ROUND5),
         "mixmom": Stat(MixMom, "mixture_moments", MIX_ROUND5), "density": Stat(Density, "chain_density", DENS_ROUND5),
         "autocorr": Stat(Autocorr, "chain_autocorr", ACF_ROUND5)}
EXPORTS = ("hmcg_version", "hmcg_device_count", "hmcg_last_error", "hmcg_shutdown",
           "hmcg_estimate_batch", "hmcg_estimate_batch_device", "hmcg_estimate_batch_multi",
           "hmcg_save_results_csv", "hmcg_write_table_csv", "hmcg_format_float") + tuple(
               "hmcg_" + s.stem + tail for s in STATS.values() for tail in ("", "_device"))


# What the library gained after include/hmcg.h was closed (version 109) is declared in companion headers and listed in companion
# tables: STATS and EXPORTS above mirror hmcg.h and stay as they are.  include/hmcg_order.h:
class Quantiles(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("device", C.c_int32),
                ("nd", C.c_int64), ("nd_ld", C.c_int64), ("Q", C.c_int32), ("flags", C.c_int32),
                ("probs", C.c_double * ORD_MAXQ)]


ORDER_EXPORTS = ("hmcg_chain_quantiles", "hmcg_chain_quantiles_device")


# include/hmcg_ergodic.h:
class Ergodic(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("W", C.c_int32), ("K", C.c_int32), ("device", C.c_int32),
                ("nd", C.c_int64), ("nd_ld", C.c_int64), ("flags", C.c_int32), ("reserved", C.c_int32)]


ERGODIC_EXPORTS = ("hmcg_ergodic_moments", "hmcg_ergodic_moments_device")


# include/hmcg_fan.h:
class Fan(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("W", C.c_int32), ("K", C.c_int32), ("device", C.c_int32),
                ("nd", C.c_int64), ("nd_ld", C.c_int64), ("n_h", C.c_int32), ("n_p", C.c_int32),
                ("horizons", C.c_int32 * HMCG_MAXH), ("rounds", C.c_int32), ("flags", C.c_int32),
                ("probs", C.c_double * FAN_MAXP), ("reserved", C.c_int64)]


FAN_EXPORTS = ("hmcg_predictive_quantiles", "hmcg_predictive_quantiles_device")


# include/hmcg_score.h:
class Score(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("W", C.c_int32), ("K", C.c_int32), ("device", C.c_int32),
                ("nd", C.c_int64), ("nd_ld", C.c_int64), ("n_h", C.c_int32), ("flags", C.c_int32),
                ("horizons", C.c_int32 * HMCG_MAXH), ("stride", C.c_int64), ("reserved", C.c_int64)]


SCORE_EXPORTS = ("hmcg_predictive_scores", "hmcg_predictive_scores_device")

_LIB = None


def build(force=False):
    """Compile libhmcgibbs.so for gfx950 with hipcc (cross-compiles without a GPU).  make decides what is stale;
    the kernel instantiations are several translation units, compiled in parallel."""
    jobs = str(max(1, min(8, len(os.sched_getaffinity(0)))))
    cmd = ["make", "-C", CSRC, "-j", jobs] + (["-B"] if force else []) + ["libhmcgibbs.so"]
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return SO_PATH


def _share_torch_hip_runtime():
    """One HIP runtime per process.  The PyTorch-ROCm wheel bundles its own libamdhip64.so
    (SONAME libamdhip64.so.7) next to libtorch_hip.so and resolves it by FILE name, while
    libhmcgibbs.so needs the SONAME.  If ours were loaded first (binding the system
    /opt/rocm runtime), a later `import torch` would bring a second runtime into the process
    and neither could use the other's device pointers or streams.  So when torch is
    installed, its copy is made resident first; libhmcgibbs then binds to it by SONAME, and
    a later `import torch` finds the same file already loaded.  Without torch (C or Julia
    callers) the system runtime is used."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    """Load the shared object (no GPU needed for this; compute calls need one)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(SO_PATH):
            raise HmcgError("libhmcgibbs.so is not built (%s); run __graft_entry__.build() -- "
                            "this package has no CPU fallback" % SO_PATH)
        _share_torch_hip_runtime()
        L = C.CDLL(SO_PATH)
        for name in EXPORTS + ORDER_EXPORTS + ERGODIC_EXPORTS + FAN_EXPORTS + SCORE_EXPORTS:
            getattr(L, name).restype = C.c_int
        L.hmcg_last_error.restype, L.hmcg_shutdown.restype = C.c_char_p, None
        _LIB = L
    return _LIB


def _check(rc):
    if rc != 0:
        msg = load().hmcg_last_error().decode("utf-8", "replace")
        raise HmcgError("libhmcgibbs rc=%d: %s" % (rc, msg))


def make_config(W, K, ldY, max_T, burnin, nrun, horizons, seed=1234, window_base=0, device=0, flags=0,
                threads_per_window=0, sweep_base=0, alpha=0.0, nu=0.0, sweep_count=0, kappa=0.0, n_samples=0,
                blend_mask=0, min_T=0):
    cfg = Config()
    cfg.struct_size = C.sizeof(Config)
    cfg.W, cfg.K, cfg.ldY, cfg.max_T = int(W), int(K), int(ldY), int(max_T)
    cfg.burnin, cfg.nrun, cfg.H = int(burnin), int(nrun), len(horizons)
    if len(horizons) > HMCG_MAXH:
        raise ValueError("at most %d horizons" % HMCG_MAXH)
    for i, h in enumerate(horizons):
        cfg.horizons[i] = int(h)
    cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    cfg.window_base = int(window_base)
    cfg.device, cfg.flags = int(device), int(flags)
    cfg.threads_per_window, cfg.sweep_base = int(threads_per_window), int(sweep_base)
    cfg.sweep_count = int(sweep_count)
    cfg.kappa, cfg.n_samples = float(kappa), int(n_samples)
    cfg.blend_mask = int(blend_mask)
    cfg.min_T = int(min_T)
    cfg.alpha, cfg.nu = float(alpha), float(nu)
    return cfg


def _np_ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _vp(x):
    """A raw device pointer or stream (an int; 0 / None: NULL) as a void pointer."""
    return None if not x else C.c_void_p(int(x))


def _device_call(fn, struct, pointers, stream, timed):
    """One *_device entry: fn(struct, pointers..., stream, timing).  Returns the Timing struct when timed, else None."""
    tm = Timing() if timed else None
    _check(fn(C.byref(struct), *[_vp(x) for x in pointers], _vp(stream), C.byref(tm) if timed else None))
    return tm


# ---- one table of a call's buffers (the Python twin of host_buffers in csrc/host_util.hpp) ----
Row = collections.namedtuple("Row", "name pos dtype shape io request carried nan")
_f64, _i32 = np.float64, np.int32
# name | position among the data pointers of hmcg_estimate_batch (None: the hmcg_extras member of that name) | dtype |
# shape, in the symbols of call_dims | in / out | the request that makes an output present (None: always; want_*: that keyword
# of build_call; draws, save_range, pif, checkpoint: see there); an input is present when it is given | a RESUME call reads
# it back | NaN in a skipped window (estimate_batch_host)
BUFFERS = tuple(Row(n, pos, dt, tuple(shape.split()), io, req, carried, nan) for n, pos, dt, shape, io, req, carried, nan in (
    ("Y",               0,    _f64,      "W ldY",      "in",  None,                  False, False),
    ("T",               1,    _i32,      "W",          "in",  None,                  False, False),
    ("yreal",           2,    _f64,      "W H",        "in",  None,                  False, False),
    ("mu",              3,    _f64,      "W K nd",     "out", "draws",               False, True),
    ("sig2",            4,    _f64,      "W K nd",     "out", "draws",               False, True),
    ("A",               5,    _f64,      "W K K nd",   "out", "draws",               False, True),
    ("pi_end",          6,    _f64,      "W K nd",     "out", "draws",               False, True),
    ("fcast",           7,    _f64,      "W 2H nd",    "out", "draws",               False, True),
    ("summary",         8,    _f64,      "W NS",       "out", None,                  False, True),
    ("status",          9,    _i32,      "W",          "out", None,                  True,  False),
    ("x_init",          None, _i32,      "W ldY",      "in",  None,                  False, False),
    ("window_ids",      None, np.uint32, "W",          "in",  None,                  False, False),
    ("sig_range",       None, _i32,      "W 2",        "in",  None,                  False, False),    # the signal Monte-Carlo path (estimatesignals!)
    ("save_range",      None, _i32,      "W 2",        "in",  None,                  False, False),
    ("sigma_signal",    None, _f64,      "W",          "in",  None,                  False, False),
    ("end_pos",         None, _i32,      "W",          "in",  None,                  False, False),    # signals past the end date (sigLen > 0)
    ("sigvals",         None, _f64,      "W ns nsave", "out", "save_range",          False, True),
    ("sample_summary",  None, _f64,      "W ns NS",    "out", "want_sample_summary", True,  True),
    ("pi_smooth_draws", None, _f64,      "W K ldY nd", "out", "want_smooth_draws",   False, True),     # samples.pib[Nrun, N, D] of every window, draw index fastest
    ("pi_smooth_mean",  None, _f64,      "W ldY K",    "out", "want_smooth",         True,  True),
    ("pi_filter_mean",  None, _f64,      "W ldY K",    "out", "want_filter_mean",    True,  True),
    ("corr",            None, _f64,      "W NC NC",    "out", "want_corr",           False, True),
    ("x_final",         None, _i32,      "W ldY",      "out", "want_state",          False, False),
    ("pif_final",       None, _f64,      "W ldY K",    "out", "pif",                 False, True),
    ("xstate",          None, np.uint8,  "W ldY",      "out", "checkpoint",          True,  False),
    ("sumacc",          None, _f64,      "W NS+K",     "out", "checkpoint",          True,  False)))
DRAW_KEYS = tuple(r.name for r in BUFFERS if r.request == "draws")
CARRIED = tuple(r.name for r in BUFFERS if r.carried)              # what a RESUME call reads back from the caller's buffers
NAN_FILLED = tuple(r.name for r in BUFFERS if r.nan)                # every float output but sumacc, the checkpoint block
ENTRY_OUTPUTS = tuple(r.name for r in BUFFERS if r.pos is not None and r.io == "out")


def call_dims(W, ldY, K, nrun, H, n_samples=0, save_range=None):
    """The dimension symbols of the BUFFERS shapes.  nd: kept draws per window (sample-major on the signal path); nsave:
    hmcg_extras.nsave_ld, the longest save_range (an int32 (W, 2) array; None: no sigvals, 0)."""
    NS, NC, ns = 3 * K + K * K + 2 * H, 3 * K + K * K + 1, max(int(n_samples), 1)
    nsave = 0 if save_range is None else int(max(1, (save_range[:, 1] - save_range[:, 0]).max()))
    return {"W": W, "ldY": ldY, "K": K, "H": H, "2H": 2 * H, "NS": NS, "NS+K": NS + K, "NC": NC, "ns": ns, "nd": ns * nrun,
            "nsave": nsave, "2": 2}


def call_shapes(dims):
    return {r.name: tuple(dims[s] for s in r.shape) for r in BUFFERS}


def build_call(store, Y, T, K, burnin, nrun, horizons=(12,), yreal=None, want_draws=True, resume=False, pif_with_smoothing=False,
               max_T=None, **kw):
    """One walk over BUFFERS for every runner: uploads the inputs that are given and allocates the outputs that are asked for
    through `store`, and returns (hmcg_config, the ten data pointers of the C entry -- None: NULL --, hmcg_extras).
    kw: the hmcg_extras inputs of BUFFERS by name, the want_* requests of its outputs, and make_config's keywords.
    store.upload(name, array, dtype) and store.alloc(name, shape, dtype) return the buffer's address; the store keeps the
    buffer and decides what it holds at first (zeros or a sentinel, an earlier call's buffer, what a RESUME call carries).
    The signal-path inputs (save_range, sigma_signal, end_pos) are ignored without sig_range.  xstate / sumacc are passed with
    want_state or resume; resume also sets HMCG_FLAG_RESUME.  Where the runners differ on purpose:
      want_draws: True, False or the names of the draw arrays to keep; the others are passed as NULL (the host runner's;
        the device runner always passes all five);
      pif_with_smoothing: pif_final is passed with any smoothing output too, not with want_state alone (the device runner's:
        the LDS-resident kernel needs it there);
      max_T, and min_T in kw: hmcg_config's (the device runner's; the host runner leaves min(max T, ldY) and 0)."""
    given = dict(Y=np.ascontiguousarray(Y, dtype=np.float64), T=T, yreal=yreal)
    W, ldY = given["Y"].shape
    given.update((r.name, kw.pop(r.name, None)) for r in BUFFERS if r.io == "in" and r.pos is None)
    if given["sig_range"] is None:
        given.update(save_range=None, sigma_signal=None, end_pos=None)
    if given["save_range"] is not None:
        given["save_range"] = np.ascontiguousarray(given["save_range"], dtype=np.int32).reshape(W, 2)
    asked = {r.request: kw.pop(r.request, False) for r in BUFFERS if str(r.request).startswith("want_")}
    smoothing = asked["want_smooth"] or asked["want_filter_mean"] or asked["want_smooth_draws"]
    asked.update({None: True, "save_range": given["save_range"] is not None, "checkpoint": asked["want_state"] or resume,
                  "pif": asked["want_state"] or (pif_with_smoothing and smoothing)})
    keep = DRAW_KEYS if want_draws is True else tuple(want_draws or ())
    shapes = call_shapes(call_dims(W, ldY, K, nrun, len(horizons), kw.get("n_samples", 0), given["save_range"]))
    ex = Extras()
    ex.struct_size, ex.nsave_ld = C.sizeof(Extras), shapes["sigvals"][2]
    args = [None] * sum(r.pos is not None for r in BUFFERS)
    for r in BUFFERS:
        if r.io == "in" and given[r.name] is not None:
            given[r.name] = np.ascontiguousarray(given[r.name], dtype=r.dtype).reshape(shapes[r.name])
            addr = store.upload(r.name, given[r.name], r.dtype)
        elif r.io == "out" and (r.name in keep if r.request == "draws" else asked[r.request]):
            addr = store.alloc(r.name, shapes[r.name], r.dtype)
        else:
            continue
        if r.pos is None:
            setattr(ex, r.name, addr)
        else:
            args[r.pos] = addr
    if max_T is None:
        max_T = min(int(given["T"].max()), ldY)
    return make_config(W, K, ldY, max_T, burnin, nrun, horizons, flags=FLAG_RESUME if resume else 0, **kw), args, ex


def timing_result(tms):
    """The timing keys of a result dict from a call's hmcg_timing records, one per device (None: an untimed call -- the
    same keys, every value None)."""
    tm = tms[0] if tms else Timing()
    out = {k: getattr(tm, k) for k in ("kernel_ms", "threads_per_window", "steps_per_thread", "lds_bytes", "helper_waves",
                                       "occupancy", "launches", "buckets")}
    out["streaming"] = bool(tm.streaming)
    out["call_ms"] = max(t.call_ms for t in tms or [tm])
    out["per_device"] = [dict(device=t.device, windows=t.windows, kernel_ms=t.kernel_ms, call_ms=t.call_ms, launches=t.launches)
                         for t in tms or []]
    return out if tms else dict.fromkeys(out)


class NumpyStore:
    """build_call's store over host arrays.  Every output starts as zeros, but: the outputs that are arguments of the C entry
    (the draws, summary, status) reuse the array of that name in `prev` -- an earlier result -- where shape, dtype and
    contiguity match, as they stand except status, which is zeroed; an output named in `carry` (a RESUME call) is a copy of it."""

    def __init__(self, prev=None, carry=None):
        self.prev, self.carry, self.inp, self.out = prev or {}, carry or {}, {}, {}

    def upload(self, name, a, dtype):
        self.inp[name] = a                   # kept alive until the call is done
        return a.ctypes.data

    def alloc(self, name, shape, dtype):
        a = self.prev.get(name) if name in ENTRY_OUTPUTS else None
        if name in self.carry:
            a = np.ascontiguousarray(self.carry[name], dtype=dtype).reshape(shape).copy()
        elif not (isinstance(a, np.ndarray) and a.shape == shape and a.dtype == dtype and a.flags.c_contiguous):
            a = np.zeros(shape, dtype=dtype)
        elif name == "status":
            a[:] = 0
        self.out[name] = a
        return a.ctypes.data


def estimate_batch_host(Y, T, K, burnin, nrun, horizons=(12,), yreal=None, seed=1234, window_base=0, device=0,
                        threads_per_window=0, x_init=None, want_state=False, want_draws=True, alpha=0.0, nu=0.0,
                        resume_state=None, sweep_base=0, window_ids=None, sweep_count=0,
                        sig_range=None, save_range=None, sigma_signal=None, kappa=0.0, n_samples=0, want_smooth=False,
                        end_pos=None, blend_mask=0, want_filter_mean=False, devices=None, out=None, want_corr=False,
                        want_sample_summary=False, resume_sample_summary=None, nan_fill=True, want_smooth_draws=False):
    """hmcg_estimate_batch over host (numpy) buffers.  Returns dict of arrays in the
    C-ABI layouts (window slowest): mu/sig2/pi_end (W,K,nrun), A (W,K,K,nrun) with
    A[w, j, i, d] = draw d of A[i,j], fcast (W,2H,nrun), summary (W,NS), status (W,).
    devices: a list of HIP ordinals -> hmcg_estimate_batch_multi (windows partitioned over those GPUs).
    out: a dict returned by an earlier call of the same shape -- its arrays are reused (a caller that owns its
    buffers, as a Julia or C caller does, pays no allocation or first-touch page faults per call).
    want_corr: out["corr"] (W, NC, NC), NC = 3K + K^2 + 1 -- the correlation matrix calccorr (src/Hmc.jl:1094-1163) builds
    per end date from the per-draw CSV files, accumulated on the device from the rounded draws (extras.corr); works with
    want_draws=False (the draws then never leave the device).
    want_sample_summary (signal path): out["sample_summary"] (W, n_samples, NS) -- per noise sample the mean over its kept
    draws of the 5-digit-rounded outputs (extras.sample_summary: the rows runaggregate makes per (date, signalid));
    resume_sample_summary carries the buffer of a call that stopped inside a sample into its RESUME call.
    resume_state: the result of the call this one continues; its status, xstate and sumacc are carried (the running smoothed /
    filtered sums are not: a host RESUME call starts them at zero)."""
    L = load()
    carry = {} if resume_state is None else {k: resume_state[k] for k in ("status", "xstate", "sumacc")}
    if resume_sample_summary is not None:
        carry["sample_summary"] = resume_sample_summary
    store = NumpyStore(out, carry)
    cfg, args, ex = build_call(
        store, Y, T, K, burnin, nrun, horizons, yreal, want_draws, resume_state is not None, seed=seed, window_base=window_base,
        device=device, threads_per_window=threads_per_window, alpha=alpha, nu=nu, kappa=kappa, n_samples=n_samples,
        blend_mask=blend_mask, sweep_base=sweep_base, sweep_count=sweep_count, x_init=x_init, window_ids=window_ids,
        sig_range=sig_range, save_range=save_range, sigma_signal=sigma_signal, end_pos=end_pos, want_state=want_state,
        want_sample_summary=want_sample_summary, want_smooth=want_smooth, want_filter_mean=want_filter_mean,
        want_smooth_draws=want_smooth_draws, want_corr=want_corr)
    args = [None if p is None else C.c_void_p(p) for p in args]
    if devices is None:
        tms = (Timing * 1)()
        rc = L.hmcg_estimate_batch(C.byref(cfg), *args, C.byref(ex), C.byref(tms[0]))
    else:
        devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        tms = (Timing * len(devices))()
        rc = L.hmcg_estimate_batch_multi(C.byref(cfg), C.c_int32(len(devices)), devs, *args, C.byref(ex), tms)
    _check(rc)
    out = store.out
    # a skipped window (non-finite data, bad T, bad ranges) was not computed: its outputs read NaN, never a
    # plausible-looking zero (the reference would have thrown, src/Hmc.jl:435)
    skipped = (out["status"] & ST_SKIPPED) != 0
    if skipped.any() and nan_fill:
        for name in NAN_FILLED:
            if name in out:
                out[name][skipped] = np.nan
    out.update(timing_result(list(tms)))
    return out


def estimate_batch_device(cfg, dY, dT, dyreal, dmu, dsig2, dA, dpi_end, dfcast, dsummary, dstatus,
                          extras=None, stream=None, timed=True):
    """hmcg_estimate_batch_device over raw device pointers (ints, e.g. torch
    tensor.data_ptr()).  Returns the Timing struct when timed, else None."""
    pointers = (dY, dT, dyreal, dmu, dsig2, dA, dpi_end, dfcast, dsummary, dstatus, C.addressof(extras) if extras is not None else None)
    return _device_call(load().hmcg_estimate_batch_device, cfg, pointers, stream, timed)


def _make_stat(name, W, cols, nd, nd_ld, device, round5, horizons=None):
    """What the structs of STATS share: struct_size, W, K or C (`cols`), device, nd, nd_ld and the ROUND5 flag; with `horizons`
    also n_h and the list (more than HMCG_MAXH raise here)."""
    if horizons is not None and len(horizons) > HMCG_MAXH:
        raise ValueError("at most %d horizons" % HMCG_MAXH)
    st = STATS[name]
    p = st.struct()
    p.struct_size = C.sizeof(st.struct)
    p.W, p.device, p.nd, p.nd_ld = int(W), int(device), int(nd), int(nd_ld)
    setattr(p, "K" if hasattr(p, "K") else "C", int(cols))
    p.flags = st.round5 if round5 else 0
    if horizons is not None:
        p.n_h = len(horizons)
        for i, h in enumerate(horizons):
            p.horizons[i] = int(h)
    return p


def _state_draws(A, **cols):
    """The per-state draw arrays of a host entry, `cols` by name with mu first, each (W, K, nd), and A (W, K, K, nd) or None, as
    contiguous float64: (arrays in the order given, A, (W, K, nd))."""
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in cols.values()]
    W, K, nd = arrs[0].shape
    if any(a.shape != arrs[0].shape for a in arrs):
        names = list(cols)
        raise ValueError("%s and %s must share the shape (W, K, nd)" % (", ".join(names[:-1]), names[-1]))
    if A is not None:
        A = np.ascontiguousarray(A, dtype=np.float64)
        if A.shape != (W, K, K, nd):
            raise ValueError("A must have the shape (W, K, K, nd)")
    return arrs, A, (W, K, nd)


def _column_draws(x, nd):
    """ONE draw array of a host entry with the draw index last, every axis between the first and the last flattened into
    columns, as contiguous float64: (x, W, columns, nd -- None: all --, leading dimension)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    W, ld = x.shape[0], x.shape[-1]
    return x, W, int(np.prod(x.shape[1:-1], dtype=np.int64)), ld if nd is None else int(nd), ld


def _tm(timing):
    """The hmcg_timing argument of a host entry: a Timing to fill, or None."""
    return C.byref(timing) if timing is not None else None


def make_predictive(W, K, nd, nd_ld, G, horizons=(0,), device=0, round5=True):
    """hmcg_predictive of a call.  More than HMCG_MAXH horizons raise here; every other rule is the library's (HMCG_E_BADARG)."""
    p = _make_stat("predictive", W, K, nd, nd_ld, device, round5, horizons)
    p.G = int(G)
    return p


def predictive_cdf_host(mu, sig2, pi_end, A, grid, horizons=(0,), device=0, round5=True, timing=None):
    """hmcg_predictive_cdf over host (numpy) draw arrays in the C-ABI layouts -- mu/sig2/pi_end (W, K, nd), A (W, K, K, nd) with
    A[w, j, i, d] = draw d of A[i, j] (None when every horizon is 0) -- as estimate_batch_host returns them.  Returns cdf
    (W, n_h, G): per window and horizon the mean over the draws of sum_k omega[k] Phi((grid[g] - mu[k]) / sqrt(sig2[k])),
    omega = pi_end A^h (calc_cdfs.jl:39-41 at h = 0).  round5 (default): every input is first rounded to 5 digits, as the cells
    of the per-draw CSV files are.  timing: a Timing to fill."""
    (mu, sig2, pi_end), A, (W, K, nd) = _state_draws(A, mu=mu, sig2=sig2, pi_end=pi_end)
    grid = np.ascontiguousarray(grid, dtype=np.float64).reshape(-1)
    p = make_predictive(W, K, nd, nd, grid.size, horizons, device, round5)
    cdf = np.zeros((W, len(horizons), grid.size))
    _check(load().hmcg_predictive_cdf(C.byref(p), _np_ptr(mu), _np_ptr(sig2), _np_ptr(pi_end), _np_ptr(A), _np_ptr(grid),
                                      _np_ptr(cdf), _tm(timing)))
    return cdf


def predictive_cdf_device(pred, dmu, dsig2, dpi_end, dA, dgrid, dcdf, stream=None, timed=False):
    """hmcg_predictive_cdf_device over raw device pointers (ints, e.g. torch tensor.data_ptr(); dA 0 / None when every horizon
    is 0); pred: make_predictive(...).  Enqueued on `stream` (None: the library's own).  Returns the Timing struct when timed
    (the call then waits for completion), else None."""
    return _device_call(load().hmcg_predictive_cdf_device, pred, (dmu, dsig2, dpi_end, dA, dgrid, dcdf), stream, timed)


def make_bias(W, K, nd, nd_ld, horizon=12, H=0, device=0, round5=True):
    """hmcg_bias of a call; every rule is the library's (HMCG_E_BADARG).  H: fcast has 2H columns per window (0 without fcast)."""
    p = _make_stat("bias", W, K, nd, nd_ld, device, round5)
    p.horizon, p.H = int(horizon), int(H)
    return p


def unpack_bias(out, K):
    """The (W, HMCG_BIAS_STRIDE(K)) output block as a dict: uncerbias (W,), totalbias (W,), mean (W, 2K) in the order
    futstate | means, cov (W, 2K, 2K) in the same order."""
    out = np.asarray(out)
    W = out.shape[0]
    return {"uncerbias": out[:, 0].copy(), "totalbias": out[:, 1].copy(), "mean": out[:, 2:2 + 2 * K].copy(),
            "cov": out[:, 2 + 2 * K:].reshape(W, 2 * K, 2 * K).copy()}


def bias_moments_host(mu, pi_end, A, fcast=None, horizon=12, device=0, round5=True, timing=None):
    """hmcg_bias_moments over host (numpy) draw arrays in the C-ABI layouts -- mu/pi_end (W, K, nd), A (W, K, K, nd) with
    A[w, j, i, d] = draw d of A[i, j] (None when horizon is 0), fcast (W, 2H, nd) or None -- as estimate_batch_host returns them.
    Returns the (W, 2 + 2K + 4K^2) block (unpack_bias names its parts): per window uncbias = nab cov nab' with upstream's
    column orders (bias_calcs.jl:49-51), totalbias = the mean of fcast[:, 1] (NaN without fcast), the mean and the covariance
    (divisor nd - 1) of [pi_end A^horizon | mu] over the draws.  round5 (default): every input is first rounded to 5 digits,
    as the cells of the per-draw CSV files are.  timing: a Timing to fill."""
    (mu, pi_end), A, (W, K, nd) = _state_draws(A, mu=mu, pi_end=pi_end)
    H = 0
    if fcast is not None:
        fcast = np.ascontiguousarray(fcast, dtype=np.float64)
        if fcast.ndim != 3 or fcast.shape[0] != W or fcast.shape[2] != nd or fcast.shape[1] % 2:
            raise ValueError("fcast must have the shape (W, 2H, nd)")
        H = fcast.shape[1] // 2
    p = make_bias(W, K, nd, nd, horizon, H, device, round5)
    out = np.zeros((W, bias_stride(K)))
    _check(load().hmcg_bias_moments(C.byref(p), _np_ptr(mu), _np_ptr(pi_end), _np_ptr(A), _np_ptr(fcast), _np_ptr(out), _tm(timing)))
    return out


def bias_moments_device(bias, dmu, dpi_end, dA, dfcast, dout, stream=None, timed=False):
    """hmcg_bias_moments_device over raw device pointers (ints, e.g. torch tensor.data_ptr(); dA 0 / None when the horizon is 0,
    dfcast 0 / None for no totalbias); bias: make_bias(...).  Enqueued on `stream` (None: the library's own).  Returns the
    Timing struct when timed (the call then waits for completion), else None."""
    return _device_call(load().hmcg_bias_moments_device, bias, (dmu, dpi_end, dA, dfcast, dout), stream, timed)


def make_mixmom(W, K, nd, nd_ld, horizons=(0,), device=0, round5=True):
    """hmcg_mixmom of a call.  More than HMCG_MAXH horizons raise here; every other rule is the library's (HMCG_E_BADARG)."""
    return _make_stat("mixmom", W, K, nd, nd_ld, device, round5, horizons)


def unpack_mixture_moments(out):
    """The (W, n_h, HMCG_MIX_STRIDE) output block as a dict of (W, n_h) arrays: mean, variance, skewness, kurtosis (excess) of
    the pooled predictive mixture, within (mean per-draw variance), between (variance over the draws of the per-draw mean,
    divisor nd), draw_skewness (mean per-draw skewness), weight (mean of sum_k omega_k)."""
    out = np.asarray(out)
    return {name: out[:, :, i].copy() for i, name in enumerate(MIX_FIELDS)}


def mixture_moments_host(mu, sig2, pi_end, A, horizons=(0,), device=0, round5=True, timing=None):
    """hmcg_mixture_moments over host (numpy) draw arrays in the C-ABI layouts -- mu/sig2/pi_end (W, K, nd), A (W, K, K, nd) with
    A[w, j, i, d] = draw d of A[i, j] (None when every horizon is 0) -- as estimate_batch_host returns them.  Returns the
    (W, n_h, 8) block (unpack_mixture_moments names its parts): per window and horizon the moments of the predictive law
    sum_k omega_k N(mu_k, sig2_k), omega = pi_end A^h, pooled over the draws in closed form (skewness.jl and alt_forecasts.jl
    asked of the draws), and its within- / between-draw split.  round5 (default): every input is first rounded to 5 digits, as
    the cells of the per-draw CSV files are.  timing: a Timing to fill."""
    (mu, sig2, pi_end), A, (W, K, nd) = _state_draws(A, mu=mu, sig2=sig2, pi_end=pi_end)
    p = make_mixmom(W, K, nd, nd, horizons, device, round5)
    out = np.zeros((W, len(horizons), MIX_STRIDE))
    _check(load().hmcg_mixture_moments(C.byref(p), _np_ptr(mu), _np_ptr(sig2), _np_ptr(pi_end), _np_ptr(A), _np_ptr(out), _tm(timing)))
    return out


def mixture_moments_device(mix, dmu, dsig2, dpi_end, dA, dout, stream=None, timed=False):
    """hmcg_mixture_moments_device over raw device pointers (ints, e.g. torch tensor.data_ptr(); dA 0 / None when every horizon
    is 0); mix: make_mixmom(...).  Enqueued on `stream` (None: the library's own).  Returns the Timing struct when timed (the
    call then waits for completion), else None."""
    return _device_call(load().hmcg_mixture_moments_device, mix, (dmu, dsig2, dpi_end, dA, dout), stream, timed)


def make_density(W, Cn, nd, nd_ld, cuts=None, bins=64, trace=(0, 1), device=0, round5=True):
    """hmcg_density of a call over a draw array of Cn columns per window.  cuts: ascending prefix lengths (None: the whole
    chain, (nd,)); trace = (length, stride) of the running mean.  More than HMCG_MAXH cuts raise here; every other rule is the
    library's (HMCG_E_BADARG)."""
    cuts = (int(nd),) if cuts is None else tuple(int(c) for c in cuts)
    if len(cuts) > HMCG_MAXH:
        raise ValueError("at most %d cuts" % HMCG_MAXH)
    p = _make_stat("density", W, Cn, nd, nd_ld, device, round5)
    p.B, p.n_cuts = int(bins), len(cuts)
    for i, c in enumerate(cuts):
        p.cuts[i] = c
    p.trace_len, p.trace_stride = int(trace[0]), int(trace[1])
    return p


def unpack_chain_density(range_, counts, stats, trace):
    """The four output blocks of hmcg_chain_density -- range (W, C, 2), counts (W, C, n_cuts, B + 3), stats (W, C, n_cuts, 2),
    trace (W, C, trace_len) -- as a dict: counts (W, C, n_cuts, B) int64 bins of the prefix d < cuts[j], below / above / nan
    (W, C, n_cuts) the draws under lo, over hi and NaN, range (W, C, 2) = (lo, hi), mean / variance (W, C, n_cuts) of the prefix
    (divisor n - 1), trace (W, C, trace_len) the running mean."""
    counts, stats = np.asarray(counts), np.asarray(stats)
    B = counts.shape[3] - 3
    return {"counts": counts[..., :B].copy(), "below": counts[..., B].copy(), "above": counts[..., B + 1].copy(),
            "nan": counts[..., B + 2].copy(), "range": np.asarray(range_).copy(), "mean": stats[..., 0].copy(),
            "variance": stats[..., 1].copy(), "trace": np.asarray(trace).copy()}


def chain_density(x, cuts=None, bins=64, lo_hi=None, trace=(0, 1), nd=None, device=0, round5=True, timing=None):
    """hmcg_chain_density over ONE host (numpy) draw array in a C-ABI layout with the draw index last -- mu / sig2 / pi_end
    (W, K, nd), A (W, K, K, nd), fcast (W, 2H, nd); every axis between the first and the last counts as columns -- over its
    first nd draws (default: all).  Per window and column: binned counts of the nested prefixes d < cuts[j] on bins equal
    widths between lo and hi (lo_hi (W, C, 2), default: the range of the finite draws), mean and variance of each prefix, and
    the running mean at (i + 1) * trace[1] draws, i < trace[0] (plots/mcplots.jl's plotchain and plotchainmean up to the
    drawing).  round5 (default): every value is first rounded to 5 digits, as the cells of the per-draw CSV files are.
    Returns the dict of unpack_chain_density, the column axis flattened.  timing: a Timing to fill."""
    x, W, Cn, nd, ld = _column_draws(x, nd)
    p = make_density(W, Cn, nd, ld, cuts, bins, trace, device, round5)
    if lo_hi is not None:
        lo_hi = np.ascontiguousarray(lo_hi, dtype=np.float64)
        if lo_hi.shape != (W, Cn, 2):
            raise ValueError("lo_hi must have the shape (W, C, 2)")
    nc, B, tl = p.n_cuts, max(int(bins), 0), max(int(trace[0]), 0)
    rng = np.zeros((W, Cn, 2))
    counts = np.zeros((W, Cn, nc, B + 3), dtype=np.int64)
    stats = np.zeros((W, Cn, nc, 2))
    tr = np.zeros((W, Cn, tl))
    _check(load().hmcg_chain_density(C.byref(p), _np_ptr(x), _np_ptr(lo_hi), _np_ptr(rng), _np_ptr(counts), _np_ptr(stats),
                                     _np_ptr(tr) if tl else None, _tm(timing)))
    return unpack_chain_density(rng, counts, stats, tr)


def chain_density_device(dens, dx, dlo_hi, drange, dcounts, dstats, dtrace, stream=None, timed=False):
    """hmcg_chain_density_device over raw device pointers (ints, e.g. torch tensor.data_ptr(); dlo_hi 0 / None for the automatic
    range, dtrace 0 / None with no trace); dens: make_density(...).  Enqueued on `stream` (None: the library's own).  Returns
    the Timing struct when timed (the call then waits for completion), else None."""
    return _device_call(load().hmcg_chain_density_device, dens, (dx, dlo_hi, drange, dcounts, dstats, dtrace), stream, timed)


def make_autocorr(W, Cn, nd, nd_ld, lags=255, device=0, round5=True):
    """hmcg_autocorr of a call over a draw array of Cn columns per window; lags = the largest lag L.  Every rule is the
    library's (HMCG_E_BADARG)."""
    p = _make_stat("autocorr", W, Cn, nd, nd_ld, device, round5)
    p.L = int(lags)
    return p


def unpack_chain_autocorr(acov, diag):
    """The two output blocks of hmcg_chain_autocorr -- acov (W, C, L + 1), diag (W, C, 8) -- as a dict: acov, the biased
    autocovariances at lags 0..L, and per (window, column) mean, variance (divisor n - 1), tau (the integrated autocorrelation
    time by Geyer's initial monotone sequence), ess = n / tau, mcse = sqrt(variance tau / n), pairs (int64: the lag pairs the
    sequence used), truncated (bool: it used every pair, the lag window is too short), rhat (split-R-hat of the two halves)."""
    diag = np.asarray(diag)
    out = {"acov": np.asarray(acov).copy()}
    for i, name in enumerate(ACF_FIELDS):
        out[name] = diag[..., i].copy()
    with np.errstate(invalid="ignore"):
        out["pairs"] = out["pairs"].astype(np.int64)
        out["truncated"] = out["truncated"] != 0.0
    return out


def chain_autocorr(x, lags=255, nd=None, device=0, round5=True, timing=None):
    """hmcg_chain_autocorr over ONE host (numpy) draw array in a C-ABI layout with the draw index last -- mu / sig2 / pi_end
    (W, K, nd), A (W, K, K, nd), fcast (W, 2H, nd); every axis between the first and the last counts as columns -- over its
    first nd draws (default: all).  Per window and column: the autocovariances at lags 0..lags and the convergence diagnostics
    of unpack_chain_autocorr.  round5 (default): every value is first rounded to 5 digits, as the cells of the per-draw CSV
    files are.  Returns the dict of unpack_chain_autocorr, the column axis flattened.  timing: a Timing to fill."""
    x, W, Cn, nd, ld = _column_draws(x, nd)
    p = make_autocorr(W, Cn, nd, ld, lags, device, round5)
    acov = np.zeros((W, Cn, max(int(lags), 0) + 1))
    diag = np.zeros((W, Cn, ACF_STRIDE))
    _check(load().hmcg_chain_autocorr(C.byref(p), _np_ptr(x), _np_ptr(acov), _np_ptr(diag), _tm(timing)))
    return unpack_chain_autocorr(acov, diag)


def chain_autocorr_device(acf, dx, dacov, ddiag, stream=None, timed=False):
    """hmcg_chain_autocorr_device over raw device pointers (ints, e.g. torch tensor.data_ptr()); acf: make_autocorr(...).
    Enqueued on `stream` (None: the library's own).  Returns the Timing struct when timed (the call then waits for completion),
    else None."""
    return _device_call(load().hmcg_chain_autocorr_device, acf, (dx, dacov, ddiag), stream, timed)


def make_quantiles(W, Cn, nd, nd_ld, probs, device=0, round5=True):
    """hmcg_quantiles of a call over a draw array of Cn columns per window.  More than ORD_MAXQ probabilities raise here; every
    other rule is the library's (HMCG_E_BADARG)."""
    probs = tuple(float(q) for q in probs)
    if len(probs) > ORD_MAXQ:
        raise ValueError("at most %d probabilities" % ORD_MAXQ)
    p = Quantiles()
    p.struct_size = C.sizeof(Quantiles)
    p.W, p.C, p.device, p.nd, p.nd_ld = int(W), int(Cn), int(device), int(nd), int(nd_ld)
    p.Q, p.flags = len(probs), ORD_ROUND5 if round5 else 0
    for i, q in enumerate(probs):
        p.probs[i] = q
    return p


def unpack_chain_quantiles(q, n):
    """The two output blocks of hmcg_chain_quantiles -- q (W, C, Q, 4), n (W, C, 2) int64 -- as a dict of (W, C, Q) arrays:
    value (the quantile), lo and hi (the order statistics x_(j) and x_(min(j + 1, m - 1)) that bracket it, bit copies of
    draws) and g (the weight of hi); plus count (W, C) int64, the m draws ranked, and nan (W, C) int64, the NaNs left out."""
    q, n = np.asarray(q), np.asarray(n)
    out = {name: q[..., i].copy() for i, name in enumerate(ORD_FIELDS)}
    out["count"], out["nan"] = n[..., 0].astype(np.int64), n[..., 1].astype(np.int64)
    return out


def chain_quantiles(x, probs, nd=None, device=0, round5=True, timing=None):
    """hmcg_chain_quantiles over ONE host (numpy) draw array in a C-ABI layout with the draw index last -- mu / sig2 / pi_end
    (W, K, nd), A (W, K, K, nd), fcast (W, 2H, nd); every axis between the first and the last counts as columns -- over its
    first nd draws (default: all).  Per window, column and probability p: the exact quantile (numpy's / Julia's default
    definition) selected on the device, with the two draws that bracket it.  round5 (default): every value is first rounded to
    5 digits, as the cells of the per-draw CSV files are.  Returns the dict of unpack_chain_quantiles, the column axis
    flattened.  timing: a Timing to fill."""
    x, W, Cn, nd, ld = _column_draws(x, nd)
    p = make_quantiles(W, Cn, nd, ld, probs, device, round5)
    q = np.zeros((W, Cn, max(p.Q, 0), ORD_STRIDE))
    n = np.zeros((W, Cn, 2), dtype=np.int64)
    _check(load().hmcg_chain_quantiles(C.byref(p), _np_ptr(x), _np_ptr(q), _np_ptr(n), _tm(timing)))
    return unpack_chain_quantiles(q, n)


def chain_quantiles_device(qs, dx, dq, dn, stream=None, timed=False):
    """hmcg_chain_quantiles_device over raw device pointers (ints, e.g. torch tensor.data_ptr()); qs: make_quantiles(...).
    Enqueued on `stream` (None: the library's own).  Returns the Timing struct when timed (the call then waits for completion),
    else None."""
    return _device_call(load().hmcg_chain_quantiles_device, qs, (dx, dq, dn), stream, timed)


def make_ergodic(W, K, nd, nd_ld, device=0, round5=True):
    """hmcg_ergodic of a call; every rule is the library's (HMCG_E_BADARG)."""
    p = Ergodic()
    p.struct_size = C.sizeof(Ergodic)
    p.W, p.K, p.device, p.nd, p.nd_ld = int(W), int(K), int(device), int(nd), int(nd_ld)
    p.flags = ERG_ROUND5 if round5 else 0
    return p


def erg_names(K):
    """The names of the HMCG_ERG_COLS(K) per-draw columns, in order."""
    return tuple("pi%d" % (k + 1) for k in range(K)) + tuple("dur%d" % (k + 1) for k in range(K)) + ("mean", "variance")


def unpack_ergodic(out, n, K, cols=None):
    """The output blocks of hmcg_ergodic_moments -- out (W, C, 2), n (W, 2) int64, C = 2K + 2 -- as a dict: per window the mean
    and the variance (divisor good - 1) over the good draws of pi (W, K) the stationary regime law, dur (W, K) the expected
    durations, mean (W,) and variance (W,) the long-run mean and variance of the series: pi_mean, pi_var, dur_mean, dur_var,
    mean_mean, mean_var, variance_mean, variance_var; good (W,) int64 the draws with all C columns finite, bad (W,) the rest;
    `cols` (W, C, nd), the per-draw columns, when they were asked for."""
    out, n = np.asarray(out), np.asarray(n)
    res = {}
    for name, sl in (("pi", slice(0, K)), ("dur", slice(K, 2 * K)), ("mean", 2 * K), ("variance", 2 * K + 1)):
        res[name + "_mean"], res[name + "_var"] = out[:, sl, 0].copy(), out[:, sl, 1].copy()
    res["good"], res["bad"] = n[:, 0].astype(np.int64), n[:, 1].astype(np.int64)
    if cols is not None:
        res["cols"] = cols
    return res


def ergodic_moments(mu, sig2, A, cols=False, nd=None, device=0, round5=True, timing=None):
    """hmcg_ergodic_moments over host (numpy) draw arrays in the C-ABI layouts -- mu/sig2 (W, K, nd), A (W, K, K, nd) with
    A[w, j, i, d] = draw d of A[i, j] -- as estimate_batch_host returns them, over their first nd draws (default: all).  Per
    draw the stationary law of the regimes (GTH elimination on the off-diagonal cells; the diagonal of A is never read), the
    expected durations and the long-run mean and variance; per window their mean and variance over the good draws.
    cols=True also returns the per-draw columns (W, 2K + 2, nd), in the layout chain_quantiles / chain_density /
    chain_autocorr take.  round5 (default): every input is first rounded to 5 digits, as the cells of the per-draw CSV files
    are.  Returns the dict of unpack_ergodic.  timing: a Timing to fill."""
    (mu, sig2), A, (W, K, ld) = _state_draws(A, mu=mu, sig2=sig2)
    if A is None:
        raise ValueError("A is required")
    nd = ld if nd is None else int(nd)
    p = make_ergodic(W, K, nd, ld, device, round5)
    Cn = erg_cols(K)
    out = np.zeros((W, Cn, 2))
    n = np.zeros((W, 2), dtype=np.int64)
    cl = np.full((W, Cn, ld), np.nan) if cols else None
    _check(load().hmcg_ergodic_moments(C.byref(p), _np_ptr(mu), _np_ptr(sig2), _np_ptr(A), _np_ptr(cl), _np_ptr(out), _np_ptr(n),
                                       _tm(timing)))
    return unpack_ergodic(out, n, K, None if cl is None else cl[:, :, :nd])


def ergodic_moments_device(erg, dmu, dsig2, dA, dcols, dout, dn, stream=None, timed=False):
    """hmcg_ergodic_moments_device over raw device pointers (ints, e.g. torch tensor.data_ptr(); dcols 0 / None when the
    per-draw columns are not kept); erg: make_ergodic(...).  Enqueued on `stream` (None: the library's own).  Returns the
    Timing struct when timed (the call then waits for completion), else None."""
    return _device_call(load().hmcg_ergodic_moments_device, erg, (dmu, dsig2, dA, dcols, dout, dn), stream, timed)


def make_fan(W, K, nd, nd_ld, probs, horizons=(0,), rounds=0, device=0, round5=True):
    """hmcg_fan of a call.  More than HMCG_MAXH horizons or FAN_MAXP probabilities raise here; every other rule is the library's
    (HMCG_E_BADARG).  rounds: 1..FAN_MAXROUNDS, 0 for the default of 4."""
    probs = tuple(float(q) for q in probs)
    if len(probs) > FAN_MAXP:
        raise ValueError("at most %d probabilities" % FAN_MAXP)
    if len(horizons) > HMCG_MAXH:
        raise ValueError("at most %d horizons" % HMCG_MAXH)
    p = Fan()
    p.struct_size = C.sizeof(Fan)
    p.W, p.K, p.device, p.nd, p.nd_ld = int(W), int(K), int(device), int(nd), int(nd_ld)
    p.n_h, p.n_p, p.rounds, p.flags = len(horizons), len(probs), int(rounds), FAN_ROUND5 if round5 else 0
    for j, h in enumerate(horizons):
        p.horizons[j] = int(h)
    for i, q in enumerate(probs):
        p.probs[i] = q
    return p


def unpack_fan(out, rng, flag):
    """The three output blocks of hmcg_predictive_quantiles -- out (W, n_h, n_p, 5), range (W, 2), flag (W, n_h, n_p) int32 -- as
    a dict: quantile, lo, hi (the last bracket), Flo, Fhi (the computed CDF at its ends), each (W, n_h, n_p); range (W, 2), the
    40-standard-deviation reach of the window's components; flag (FAN_NAN | FAN_UNREACHED | FAN_FLAT)."""
    out = np.asarray(out)
    res = {name: out[..., i].copy() for i, name in enumerate(FAN_FIELDS)}
    res["range"], res["flag"] = np.asarray(rng).copy(), np.asarray(flag).copy()
    return res


def predictive_quantiles(mu, sig2, pi_end, A, probs, horizons=(0,), rounds=0, nd=None, device=0, round5=True, timing=None):
    """hmcg_predictive_quantiles over host (numpy) draw arrays in the C-ABI layouts -- mu/sig2/pi_end (W, K, nd), A (W, K, K, nd)
    with A[w, j, i, d] = draw d of A[i, j] (None when every horizon is 0) -- as estimate_batch_host returns them, over their first
    nd draws (default: all).  Per window, horizon and probability p the quantile of the predictive law, the mixture of nd * K
    normals whose CDF predictive_cdf_host evaluates: the median, the forecast bands of a fan chart, value-at-risk levels.  The
    CDF is inverted by grid refinement, `rounds` rounds (default 4: |F(q) - p| below 1e-10).  round5 (default): every input is
    first rounded to 5 digits, as the cells of the per-draw CSV files are.  Returns the dict of unpack_fan.  timing: a Timing to
    fill."""
    (mu, sig2, pi_end), A, (W, K, ld) = _state_draws(A, mu=mu, sig2=sig2, pi_end=pi_end)
    nd = ld if nd is None else int(nd)
    p = make_fan(W, K, nd, ld, probs, horizons, rounds, device, round5)
    out = np.zeros((W, p.n_h, p.n_p, FAN_STRIDE))
    rng = np.zeros((W, 2))
    flag = np.zeros((W, p.n_h, p.n_p), dtype=np.int32)
    _check(load().hmcg_predictive_quantiles(C.byref(p), _np_ptr(mu), _np_ptr(sig2), _np_ptr(pi_end), _np_ptr(A), _np_ptr(out),
                                            _np_ptr(rng), _np_ptr(flag), _tm(timing)))
    return unpack_fan(out, rng, flag)


def predictive_quantiles_device(fan, dmu, dsig2, dpi_end, dA, dout, drange, dflag, stream=None, timed=False):
    """hmcg_predictive_quantiles_device over raw device pointers (ints, e.g. torch tensor.data_ptr(); dA 0 / None when every
    horizon is 0); fan: make_fan(...).  Enqueued on `stream` (None: the library's own).  Returns the Timing struct when timed
    (the call then waits for completion), else None."""
    return _device_call(load().hmcg_predictive_quantiles_device, fan, (dmu, dsig2, dpi_end, dA, dout, drange, dflag), stream, timed)


def score_thinning(nd, stride=0):
    """(stride, n_u) of a score call over nd draws: the draws u * stride, u < n_u = ceil(nd / stride), are used; stride 0 is the
    default, the smallest stride that leaves at most SCORE_DRAWS_DEFAULT draws."""
    nd, stride = int(nd), int(stride)
    if stride <= 0:
        stride = max(1, -(-nd // SCORE_DRAWS_DEFAULT))
    return stride, -(-nd // stride)


def make_score(W, K, nd, nd_ld, horizons=(0,), stride=0, device=0, round5=True):
    """hmcg_score of a call.  More than HMCG_MAXH horizons raise here; every other rule is the library's (HMCG_E_BADARG).
    stride: every stride-th draw is used, 0 for the default thinning (at most 4 096 draws), 1 for the exact score."""
    if len(horizons) > HMCG_MAXH:
        raise ValueError("at most %d horizons" % HMCG_MAXH)
    p = Score()
    p.struct_size = C.sizeof(Score)
    p.W, p.K, p.device, p.nd, p.nd_ld = int(W), int(K), int(device), int(nd), int(nd_ld)
    p.n_h, p.flags, p.stride = len(horizons), SCORE_ROUND5 if round5 else 0, int(stride)
    for j, h in enumerate(horizons):
        p.horizons[j] = int(h)
    return p


def unpack_scores(out, yreal=None):
    """The (W, n_h, 5) output block of hmcg_predictive_scores as a dict of (W, n_h) arrays: crps, e_abs = E|X - y|, e_pair =
    E|X - X'| (the forecast's Gini mean difference), pit = F(y), pdf = F'(y); plus yreal (W, n_h) when given as (n_h, W)."""
    out = np.asarray(out)
    res = {name: out[..., i].copy() for i, name in enumerate(SCORE_FIELDS)}
    if yreal is not None:
        res["yreal"] = np.asarray(yreal).T.copy()
    return res


def _score_yreal(yreal, n_h, W):
    """yreal as the (n_h, W) float64 block of the ABI; None: all unknown (NaN)."""
    if yreal is None:
        return np.full((n_h, W), np.nan)
    yreal = np.ascontiguousarray(yreal, dtype=np.float64)
    if yreal.shape != (n_h, W):
        raise ValueError("yreal must have the shape (n_h, W) = (%d, %d)" % (n_h, W))
    return yreal


def predictive_scores(mu, sig2, pi_end, A, yreal, horizons=(0,), stride=0, nd=None, device=0, round5=True, timing=None):
    """hmcg_predictive_scores over host (numpy) draw arrays in the C-ABI layouts -- mu/sig2/pi_end (W, K, nd), A (W, K, K, nd)
    with A[w, j, i, d] = draw d of A[i, j] (None when every horizon is 0) -- as estimate_batch_host returns them, over their first
    nd draws (default: all).  yreal (n_h, W): the realised value per horizon and window, NaN for unknown (None: all unknown).
    Per window and horizon the continuous ranked probability score of the predictive law (the mixture of n_u * K normals whose
    CDF predictive_cdf_host evaluates, n_u the draws the thinning leaves: score_thinning) against yreal, its two parts, the
    probability integral transform and the predictive density at yreal.  round5 (default): every draw input is first rounded to
    5 digits, as the cells of the per-draw CSV files are.  Returns the dict of unpack_scores.  timing: a Timing to fill."""
    (mu, sig2, pi_end), A, (W, K, ld) = _state_draws(A, mu=mu, sig2=sig2, pi_end=pi_end)
    nd = ld if nd is None else int(nd)
    p = make_score(W, K, nd, ld, horizons, stride, device, round5)
    yreal = _score_yreal(yreal, p.n_h, W)
    out = np.zeros((W, p.n_h, SCORE_STRIDE))
    _check(load().hmcg_predictive_scores(C.byref(p), _np_ptr(mu), _np_ptr(sig2), _np_ptr(pi_end), _np_ptr(A), _np_ptr(yreal),
                                         _np_ptr(out), _tm(timing)))
    return unpack_scores(out, yreal)


def predictive_scores_device(score, dmu, dsig2, dpi_end, dA, dyreal, dout, stream=None, timed=False):
    """hmcg_predictive_scores_device over raw device pointers (ints, e.g. torch tensor.data_ptr(); dA 0 / None when every horizon
    is 0); score: make_score(...).  Enqueued on `stream` (None: the library's own).  Returns the Timing struct when timed (the
    call then waits for completion), else None."""
    return _device_call(load().hmcg_predictive_scores_device, score, (dmu, dsig2, dpi_end, dA, dyreal, dout), stream, timed)


def format_float(x):
    """CSV.jl 0.5.16 text of one Float64 (hmcg_format_float)."""
    buf = C.create_string_buffer(48)
    n = load().hmcg_format_float(C.c_double(float(x)), buf)
    return buf.raw[:n].decode()


def save_results_csv(dir, dates, K, horizons, res, sigvals=None, nsave=0, legacy_trans_header=False, n_threads=0):
    """hmcg_save_results_csv: the five per-window CSV files of saveresults (src/Hmc.jl:724-748) for every window of a
    result dict of estimate_batch_host (C-ABI layouts), written by the library's native writer."""
    W = len(dates)
    H = len(horizons)
    os.makedirs(dir, exist_ok=True)

    def arr(name, shape):
        a = res.get(name)
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.shape == shape, (name, a.shape, shape)
        return a
    nd = next(res[k].shape[-1] for k in ("mu", "sig2", "pi_end", "A", "fcast") if res.get(k) is not None)
    mu, sig2, pe = arr("mu", (W, K, nd)), arr("sig2", (W, K, nd)), arr("pi_end", (W, K, nd))
    A, fc = arr("A", (W, K, K, nd)), arr("fcast", (W, 2 * H, nd))
    dts = (C.c_char_p * W)(*[str(d).encode() for d in dates])
    hz = (C.c_int32 * max(H, 1))(*[int(h) for h in horizons])
    sv = None
    n_samples = nsave_ld = 0
    if sigvals is not None:
        sv = np.ascontiguousarray(sigvals, dtype=np.float64)
        _, n_samples, nsave_ld = sv.shape
    rc = load().hmcg_save_results_csv(str(dir).encode(), C.c_int32(W), dts, C.c_int32(K), C.c_int32(H), hz, C.c_int64(nd),
                                      _np_ptr(mu), _np_ptr(sig2), _np_ptr(pe), _np_ptr(A), _np_ptr(fc), _np_ptr(sv),
                                      C.c_int32(n_samples), C.c_int32(nsave), C.c_int32(nsave_ld),
                                      C.c_int32(1 if legacy_trans_header else 0), C.c_int32(n_threads))
    if rc != 0:
        raise HmcgError("hmcg_save_results_csv rc=%d (directory %s)" % (rc, dir))
