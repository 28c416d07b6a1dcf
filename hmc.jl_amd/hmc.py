"""Host-side mirror of the reference's `module Hmc` surface for the hot path.

Julia is not available in the build image, so the tested host layer is this Python
module; `julia/Hmc.jl` carries the same surface as a Julia module over the same C
ABI.  Names, argument meaning and result layout follow the reference:

    estopt              src/Hmc.jl:17-73     (fields and keyword defaults)
    makey/startdate/enddate/yobs/yend   src/Hmc.jl:85-107
    makedate            src/Hmc.jl:573-582
    estimatemodel       src/Hmc.jl:850-865   -> (mu, sigma, pib, A, forecasts, obsdates)
    estimatesignals     src/Hmc.jl:868-914   (estimatesignals!; signal ranges ending at endIndex)
    forecast            src/Hmc.jl:658-667
    saveresults/basicsave   src/Hmc.jl:707-748   (five per-window CSVs)
    runaggregate layout src/Hmc.jl:1025-1078 (`*_summary.csv`)
    calccorr            src/Hmc.jl:1094-1163 (correlations.xlsx; matrices from the files or from the device)
    calccdfs            code/hassan_cdfs/calc_cdfs.jl:31-42 (predictive CDFs; from the files or from the device)
    calcbias            code/hassan_cdfs/bias_calcs.jl:40-53 (uncerbias / totalbias; from the files or from the device)
    calcskewness        code/skewness.jl:22-43 (the plug-in mixture's skewness, in closed form instead of 10 000 000 variates)
    altforecasts        code/alt_forecasts.jl:23-39 (plug-in against proper 12-month forecast; forecast_comparision.csv)
    calcmoments         both questions asked of the draws: moments of the predictive mixture (from the files or from the device)
    calcchain           plots/mcplots.jl:24-63 and plots/timeseriesplots.jl:83-142 up to the drawing: binned chain densities over
                        nested prefixes and the running mean (from the files or from the device); chainquantiles, chaindensity
    calcess             no reference script: autocovariances, integrated autocorrelation time, effective sample size, Monte-Carlo
                        standard error and split-R-hat of the draws (from the files or from the device); write_chain_ess
    calcquantiles       no reference script: exact quantiles (median, credible limits) of the draws by selection (from the files
                        or from the device); write_chain_quantiles
    calcergodic         no reference script: the stationary regime law, expected durations and long-run mean and variance of
                        the draws, the limit of pi_end A^h (from the files or from the device); write_ergodic
    calcfan             no reference script (calc_cdfs.jl only plots `finverse`): quantiles of the predictive regime mixture --
                        median, forecast bands, value at risk -- per end date and horizon (from the files or from the
                        device); write_fan
    calcscores          no reference script (the reference verifies the point forecast alone): the continuous ranked probability
                        score of the predictive regime mixture against the realised value, the probability integral transform
                        and the predictive density, per end date and horizon (from the files or from the device);
                        write_scores, scoresummary

New (the reference batches by launching one SLURM task per window,
slurmscripts/base_estimation.sh:5): `estimatewindows`, one call for many windows.

All sampling runs in libhmcgibbs (HIP, gfx950).  No CPU fallback.
"""
import datetime as _dt
import math
import os
import numpy as np

from . import _lib

class Samples:
    """The NamedTuple estimatemodel returns upstream (src/Hmc.jl:864): fields μ, σ, πb, A,
    forecasts, obsdates (ASCII aliases mu, sigma, pib), plus the window's status word."""

    def __init__(self, μ, σ, πb, A, forecasts, obsdates, status=0, signalvals=None, signalids=None):
        self.μ, self.σ, self.πb, self.A = μ, σ, πb, A
        self.forecasts, self.obsdates, self.status = forecasts, obsdates, status
        self.signalvals, self.signalids = signalvals, signalids      # estimatesignals! only (src/Hmc.jl:913)

    mu = property(lambda s: s.μ)
    sigma = property(lambda s: s.σ)
    pib = property(lambda s: s.πb)


def makedate(x):
    """Stata monthly date (months since 1960-01) -> date (src/Hmc.jl:573-582)."""
    y = int(x)
    return _dt.date(y // 12 + 1960, y % 12 + 1, 1)


class estopt:
    """Run options; field names and defaults of the reference struct (src/Hmc.jl:17-60).

    Index ranges are 1-based inclusive `range` objects or sequences, as in Julia
    (sampleRange=range(1, 122) is Julia's 1:121).  As in the reference, windows are
    expected to start at index 1."""

    def __init__(self, rawdata, dates, sampleRange=range(1, 122), signalRange=range(2, 2), signalSave=range(2, 2),
                 endIndex=121, horizons=(12,), D=3, burnin=1000, Nrun=1000, signalburnin=1000, signalNrun=1000,
                 noise=0.0, noiseSamples=1, σsignal=0.0, series="offical", seed=1234):
        self.rawdata = np.asarray(rawdata, dtype=np.float64)
        self.dates = list(dates)
        self.sampleRange = list(sampleRange)
        self.signalRange = list(signalRange)
        self.signalSave = list(signalSave)
        if not set(self.signalRange) <= set(self.sampleRange):
            print("ERROR: signalRange is not a subset of sampleRange")     # @error only logs (src/Hmc.jl:61)
        if not set(self.signalSave) <= set(self.signalRange):
            print("ERROR: signalSave is not a subset of signalRange")      # src/Hmc.jl:62
        self.endIndex = int(endIndex)
        self.horizons = list(horizons)
        self.D = int(D)
        self.burnin = int(burnin)
        self.Nrun = int(Nrun)
        self.signalburnin = int(signalburnin)
        self.signalNrun = int(signalNrun)
        self.noise = float(noise)
        self.noiseSamples = int(noiseSamples)
        self.σsignal = float(σsignal)
        self.series = series
        self.seed = int(seed)
        update_itators(self)


def update_itators(opt):
    """src/Hmc.jl:75-83 (the reference's spelling is kept)."""
    sig = set(opt.signalRange)
    opt.obsRange = [i for i in opt.sampleRange if i not in sig]


def makey(opt):
    return opt.rawdata[np.asarray(opt.sampleRange, dtype=np.int64) - 1]


def enddate(opt, extra=0):
    return opt.dates[opt.endIndex + extra - 1]


def startdate(opt):
    return opt.dates[opt.sampleRange[0] - 1]


def yobs(opt, index):
    return opt.rawdata[index - 1]


def yend(opt, extra=0):
    return opt.rawdata[opt.endIndex + extra - 1]


def forecast(μ, A, πb, horizon, Yreal):
    """(pi' A^h) . mu and its error (src/Hmc.jl:658-667).  Host arithmetic on one draw,
    kept for API parity; per-draw forecasts inside estimatemodel come from the GPU."""
    S1 = np.asarray(πb, dtype=np.float64) @ np.linalg.matrix_power(np.asarray(A, dtype=np.float64), int(horizon))
    f = float(S1 @ np.asarray(μ, dtype=np.float64))
    return f, f - Yreal


def _yreal_row(rawdata, endIndex, horizons):
    out = np.full(len(horizons), np.nan)
    for i, h in enumerate(horizons):
        j = endIndex + h
        if 1 <= j <= len(rawdata):
            out[i] = rawdata[j - 1]
    return out


def _check_live_path(opt):
    if opt.sampleRange[0] != 1 or opt.sampleRange != list(range(1, opt.sampleRange[-1] + 1)):
        raise ValueError("sampleRange must be 1:N (the reference indexes window-relative arrays with absolute "
                         "indices, src/Hmc.jl:254,406 -- only windows starting at 1 are meaningful)")
    sr = opt.signalRange
    if len(sr):
        if sr != list(range(sr[0], sr[-1] + 1)) or sr[-1] != opt.sampleRange[-1]:
            raise NotImplementedError("signalRange must be a contiguous tail of sampleRange")
        if not 0 <= sr[-1] - opt.endIndex <= _lib.HMCG_MAXTAIL:
            raise NotImplementedError("sigLen = last(signalRange) - endIndex (src/Hmc.jl:888) must lie in 0..%d"
                                      % _lib.HMCG_MAXTAIL)


def _sig_ranges(opt):
    """0-based half-open (signal, save) position ranges of the window, or (None, None)."""
    if not len(opt.signalRange):
        return None, None
    sig = (opt.signalRange[0] - 1, opt.signalRange[-1])
    sv = (opt.signalSave[0] - 1, opt.signalSave[-1]) if len(opt.signalSave) else (0, 0)
    return sig, sv


def _check_status(status, what):
    """Per-window status words of a finished call: a window the library skipped is an error here, as it is upstream
    (a NaN observation or an empty window makes the reference throw, src/Hmc.jl:435,464); the numerical flags only warn."""
    import warnings
    status = np.atleast_1d(np.asarray(status))
    bad = np.nonzero(status & _lib.ST_SKIPPED)[0]
    if len(bad):
        names = {_lib.ST_NONFINITE: "non-finite observation", _lib.ST_BAD_T: "window length / end position out of range",
                 _lib.ST_BAD_RANGE: "signal or save range out of range"}
        why = sorted({n for w in bad for b, n in names.items() if status[w] & b})
        raise _lib.HmcgError("%s: window(s) %s were not estimated (%s); their outputs are NaN"
                             % (what, ", ".join(str(int(w)) for w in bad[:8]), "; ".join(why)))
    other = np.nonzero(status)[0]
    if len(other):
        warnings.warn("%s: numerical flags raised in %d window(s) (status bits %s): see HMCG_ST_* in include/hmcg.h"
                      % (what, len(other), sorted({int(s) for s in status[other]})), RuntimeWarning, stacklevel=3)


# RNG stream of estimatesignals!' base run (:869-872): window id with the top bit set, so that the base chain and the
# first noise sample -- same seed, same window, same sweep numbers -- do not replay the same Philox counters
# (upstream's single MersenneTwister stream simply continues from one run into the next)
BASE_RUN_STREAM = 0x80000000


def _unpack(res, w, nrun, K, H, obsdate):
    mu = res["mu"][w].T.copy()                       # (nrun, K)
    sig = res["sig2"][w].T.copy()
    pe = res["pi_end"][w].T.copy()
    A = np.transpose(res["A"][w], (2, 1, 0)).copy()  # [d, i, j]
    fc = res["fcast"][w].T.copy() if H else np.zeros((nrun, 0))
    return Samples(mu, sig, pe[:, None, :], A, fc, [obsdate] * nrun, int(res["status"][w]))


def estimatemodel(opt, device=0, smooth=False, window_id=0):
    """Hmc.estimatemodel(opt) (src/Hmc.jl:850-865) on the GPU.

    smooth="draws" returns the reference's full samples.πb[Nrun, N, D] (every kept draw's smoothed probabilities,
    backwardupdate_P!, :442-457, stored per draw :558) -- 8 N D bytes per draw -- besides πb_mean / πf_mean.

    smooth=True additionally runs the full backward pass (backwardupdate_P!, :442-457) every sweep and
    returns, as `samples.πb_mean` (N, D), the mean over the kept draws of the smoothed probabilities
    `samples.πb[:, t, :]` -- what smoothStates/forecastinsample average upstream (:649-654, :696).

    Returns Samples(μ[Nrun,D], σ[Nrun,D] (variances), πb[Nrun,1,D], A[Nrun,D,D],
    forecasts[Nrun,2H], obsdates).  πb keeps only the window's last time step -- the
    only slice the reference's outputs consume (`samples.πb[:,end,:]`, src/Hmc.jl:744,861)
    -- so `samples.πb[:, -1, :]` reads exactly as upstream.

    If opt carries a signal range the call is the base run of estimatesignals! (:869-872): upstream
    builds HyperParams(Y, D) there, i.e. alpha = nu = 1 and kappa = 1.0 whatever opt.noise says."""
    _check_live_path(opt)
    Y = makey(opt)
    sig, sv = _sig_ranges(opt)
    kw = {}
    if sig is not None:
        kw = dict(sig_range=[sig], save_range=[sv], sigma_signal=[0.0], kappa=1.0, n_samples=1)
    res = _lib.estimate_batch_host(Y[None, :], [len(Y)], opt.D, opt.burnin, opt.Nrun, tuple(opt.horizons),
                                   _yreal_row(opt.rawdata, opt.endIndex, opt.horizons)[None, :], seed=opt.seed,
                                   device=device, want_smooth=bool(smooth), want_filter_mean=bool(smooth), window_ids=[window_id],
                                   want_smooth_draws=(smooth == "draws"), **kw)
    _check_status(res["status"], "estimatemodel")
    s = _unpack(res, 0, opt.Nrun, opt.D, len(opt.horizons), enddate(opt))
    if smooth == "draws":
        s.πb = np.ascontiguousarray(np.transpose(res["pi_smooth_draws"][0, :, :len(Y), :], (2, 1, 0)))     # (Nrun, N, D), as upstream
    if smooth:
        s.πb_mean = res["pi_smooth_mean"][0, :len(Y)]
        s.πf_mean = res["pi_filter_mean"][0, :len(Y)]      # draw-averaged filtered probabilities (sorted labels)
    return s


def savesmoothresults(πb_mean, dates, dir):
    """`smoothed_state_probs.csv` in the layout of savesmoothresults (src/Hmc.jl:750-758): Date, state_1.."""
    os.makedirs(dir, exist_ok=True)
    D = πb_mean.shape[1]
    with open(os.path.join(dir, "smoothed_state_probs.csv"), "w") as f:
        f.write(",".join(["Date"] + ["state_%d" % i for i in range(1, D + 1)]) + "\n")
        for d, row in zip(dates, πb_mean):
            f.write(",".join([str(d)] + [_fmt(v) for v in row]) + "\n")


def estimatesignals(opt, device=0):
    """Hmc.estimatesignals!(opt) (src/Hmc.jl:868-914) on the GPU (the `!`: opt.σsignal is set when it was 0).

    opt.noiseSamples chains of signalburnin + signalNrun sweeps run back to back on
    Yfake = Yreal + N(0,1) * σsignal over opt.signalRange, the chain state carried from one noise sample
    to the next as upstream (:889-895), with HyperParams(opt): alpha = nu = 2, kappa = opt.noise (:148-159).
    Returns Samples with (noiseSamples*signalNrun) draws, sample-major, plus signalvals[Ndraws, len(signalSave)]
    and signalids[Ndraws] (1-based), as the reference's NamedTuple (:913).  The noise comes from this
    library's counter-based RNG (site 5), not Julia's stream.

    Signals past the end date (sigLen = last(signalRange) - endIndex > 0, :888; the len_1 / len_12 experiments of
    code/run_hmm.jl:122-158): πb is the SMOOTHED probability at endIndex (:900); a horizon h > sigLen is forecast
    h - sigLen steps from the window's last step (:906-907), h == sigLen goes through forecastsignal (:908-909)
    and h < sigLen is left unset upstream (uninitialised memory) -- NaN here."""
    _check_live_path(opt)
    if not len(opt.signalRange):
        raise ValueError("estimatesignals needs a signalRange")
    if opt.σsignal == 0:                                   # isapprox(opt.σsignal, 0) (:869)
        base = estimatemodel(opt, device=device, window_id=BASE_RUN_STREAM)
        opt.σsignal = float(np.mean(base.σ)) * opt.noise  # :871
    Y = makey(opt)
    sig, sv = _sig_ranges(opt)
    n, ns = opt.signalNrun, opt.noiseSamples
    sigLen = opt.signalRange[-1] - opt.endIndex                                 # :888
    dev_h = [h - sigLen if h > sigLen else 0 for h in opt.horizons]             # :907
    blend = sum(1 << k for k, h in enumerate(opt.horizons) if h == sigLen and sigLen > 0)
    unset = [k for k, h in enumerate(opt.horizons) if h < sigLen]
    kw = dict(end_pos=[opt.endIndex - 1], blend_mask=blend) if sigLen > 0 else {}
    res = _lib.estimate_batch_host(Y[None, :], [len(Y)], opt.D, opt.signalburnin, n, tuple(dev_h),
                                   _yreal_row(opt.rawdata, opt.endIndex, opt.horizons)[None, :], seed=opt.seed,
                                   device=device, sig_range=[sig], save_range=[sv], sigma_signal=[opt.σsignal],
                                   kappa=opt.noise, n_samples=ns, alpha=2.0, nu=2.0, **kw)
    _check_status(res["status"], "estimatesignals")
    for k in unset:
        res["fcast"][0, 2 * k:2 * k + 2] = np.nan
    s = _unpack(res, 0, ns * n, opt.D, len(opt.horizons), enddate(opt))
    nsave = len(opt.signalSave)
    s.signalvals = np.repeat(res["sigvals"][0][:, :nsave], n, axis=0)           # :904
    s.signalids = np.repeat(np.arange(1, ns + 1), n)                            # :903
    return s


def estimatesignalswindows(opts, device=0, window_ids=None, keep_draws=True, summaries=False):
    """estimatesignals! for many windows in one GPU call (what the reference fans out as one SLURM task per end date,
    slurmscripts/base_estimation.sh:5): opts is a list of estopt with signal ranges that share D, horizons, the sweep
    counts, noiseSamples, noise, seed and sigLen.  Windows whose opt.σsignal is 0 get it from a batched base run first
    (:869-872).  Returns the list of Samples in the order of opts.  RNG stream ids default to the position in `opts`
    (pass window_ids = zeros to reproduce single-window estimatesignals calls draw for draw).
    summaries=True additionally returns, as a second value, a dict with `sample_summary` (W, noiseSamples, 3K+K^2+2H) -- per
    noise sample the mean of its signalNrun rounded draws, taken on the device: the rows runaggregate(datadir, var) makes per
    (date, signalid) (src/Hmc.jl:1053-1075); write_signal_summaries writes them as upstream's files -- and `signalvals`
    (W, noiseSamples, len(signalSave)).  With keep_draws=False no draw leaves the GPU and the first value is None."""
    o0 = opts[0]
    W = len(opts)
    for o in opts:
        _check_live_path(o)
        if not len(o.signalRange):
            raise ValueError("estimatesignalswindows needs a signalRange in every window")
        same = (o.D, tuple(o.horizons), o.burnin, o.Nrun, o.signalburnin, o.signalNrun, o.noiseSamples, o.noise, o.seed,
                o.signalRange[-1] - o.endIndex, len(o.signalSave))
        if same != (o0.D, tuple(o0.horizons), o0.burnin, o0.Nrun, o0.signalburnin, o0.signalNrun, o0.noiseSamples, o0.noise,
                    o0.seed, o0.signalRange[-1] - o0.endIndex, len(o0.signalSave)):
            raise ValueError("windows of one call must share D, horizons, sweep counts, noise settings, seed and sigLen")
    Tw = np.array([len(o.sampleRange) for o in opts], dtype=np.int32)
    ld = int(Tw.max())
    Y = np.zeros((W, ld))
    for w, o in enumerate(opts):
        Y[w, :Tw[w]] = makey(o)
    yreal = np.stack([_yreal_row(o.rawdata, o.endIndex, o.horizons) for o in opts])
    sig = np.array([_sig_ranges(o)[0] for o in opts], dtype=np.int32)
    sv = np.array([_sig_ranges(o)[1] for o in opts], dtype=np.int32)
    wid = np.arange(W, dtype=np.uint32) if window_ids is None else np.asarray(window_ids, dtype=np.uint32)
    need = [w for w, o in enumerate(opts) if o.σsignal == 0]
    if need:                                               # base runs (:869-872): kappa = 1, alpha = nu = 1, no noise
        idx = np.array(need)
        base = _lib.estimate_batch_host(Y[idx], Tw[idx], o0.D, o0.burnin, o0.Nrun, tuple(o0.horizons), yreal[idx], seed=o0.seed,
                                        device=device, want_draws=("sig2",), window_ids=wid[idx] | np.uint32(BASE_RUN_STREAM), sig_range=sig[idx],
                                        save_range=sv[idx], sigma_signal=np.zeros(len(idx)), kappa=1.0, n_samples=1)
        _check_status(base["status"], "estimatesignalswindows (base run)")
        for i, w in enumerate(need):
            opts[w].σsignal = float(np.mean(base["sig2"][i].T.copy())) * opts[w].noise     # :871 (summed as estimatesignals does)
    n, ns = o0.signalNrun, o0.noiseSamples
    sigLen = o0.signalRange[-1] - o0.endIndex
    dev_h = [h - sigLen if h > sigLen else 0 for h in o0.horizons]
    blend = sum(1 << k for k, h in enumerate(o0.horizons) if h == sigLen and sigLen > 0)
    kw = dict(end_pos=[o.endIndex - 1 for o in opts], blend_mask=blend) if sigLen > 0 else {}
    res = _lib.estimate_batch_host(Y, Tw, o0.D, o0.signalburnin, n, tuple(dev_h), yreal, seed=o0.seed, device=device,
                                   window_ids=wid, sig_range=sig, save_range=sv, sigma_signal=[o.σsignal for o in opts],
                                   kappa=o0.noise, n_samples=ns, alpha=2.0, nu=2.0, want_draws=bool(keep_draws),
                                   want_sample_summary=bool(summaries), **kw)
    _check_status(res["status"], "estimatesignalswindows")
    nsave = len(o0.signalSave)
    NP = 3 * o0.D + o0.D * o0.D
    extra = None
    if summaries:
        ss = res["sample_summary"].copy()
        for k, h in enumerate(o0.horizons):
            if h < sigLen:
                ss[:, :, NP + 2 * k:NP + 2 * k + 2] = np.nan
        extra = dict(sample_summary=ss, signalvals=res["sigvals"][:, :, :nsave].copy())
    if not keep_draws:
        return None, extra
    for k, h in enumerate(o0.horizons):
        if h < sigLen:
            res["fcast"][:, 2 * k:2 * k + 2] = np.nan
    out = []
    for w, o in enumerate(opts):
        s = _unpack(res, w, ns * n, o.D, len(o.horizons), enddate(o))
        s.signalvals = np.repeat(res["sigvals"][w][:, :nsave], n, axis=0)
        s.signalids = np.repeat(np.arange(1, ns + 1), n)
        out.append(s)
    return (out, extra) if summaries else out


class BiasMoments:
    """bias_calcs.jl's numbers per window: uncerbias (W,), totalbias (W,), and the moments behind them, mean (W, 2K) and
    cov (W, 2K, 2K) of [pi_end A^horizon | mu] over the draws, both in the order futstate | means."""

    def __init__(self, horizon, uncerbias, totalbias, mean, cov):
        self.horizon, self.uncerbias, self.totalbias, self.mean, self.cov = int(horizon), uncerbias, totalbias, mean, cov


class MixtureMoments:
    """Moments of the predictive law sum_k omega_k N(mu_k, sig2_k), omega = pi_end A^h, pooled over a window's draws: (W, n_h)
    arrays mean, variance, skewness, kurtosis (excess), within (mean per-draw variance), between (variance over the draws of
    the per-draw mean), draw_skewness (mean per-draw skewness), weight (mean of sum_k omega_k); horizons: the n_h horizons."""

    def __init__(self, horizons, parts):
        self.horizons = tuple(int(h) for h in horizons)
        for name in _lib.MIX_FIELDS:
            setattr(self, name, parts[name])


DENSITY_FILES = {"mu": "filtered_means", "sig2": "filtered_variances", "pi_end": "filtered_state_probs",
                 "A": "filtered_trans_probs", "fcast": "forecasts"}


class ChainDensity:
    """Chain densities of one variable's draws over n windows (end dates), C columns and the nested prefixes d < cuts[j]:
    counts (n, C, n_cuts, bins) int64 on `bins` equal-width bins between range[..., 0] and range[..., 1]; below, above, nan
    (n, C, n_cuts) the draws under lo, over hi and NaN; mean, variance (n, C, n_cuts) of each prefix (divisor n - 1);
    trace (n, C, trace_len) the running mean after (i + 1) * trace_stride draws; columns: the C column names of the per-draw
    file."""

    def __init__(self, var, columns, cuts, trace_stride, parts):
        self.var, self.columns, self.cuts, self.trace_stride = var, list(columns), tuple(int(c) for c in cuts), int(trace_stride)
        for name in _lib.DENS_FIELDS:
            setattr(self, name, parts[name])
        self.bins = int(self.counts.shape[3])

    def rows(self, idx):
        """The same object restricted to the windows idx."""
        return ChainDensity(self.var, self.columns, self.cuts, self.trace_stride, {k: getattr(self, k)[idx] for k in _lib.DENS_FIELDS})


class ChainAutocorr:
    """Autocovariances and convergence diagnostics of one variable's draws over n windows (end dates) and C columns: acov
    (n, C, lags + 1) the biased autocovariances at lags 0..lags; mean, variance (divisor n - 1), tau (integrated autocorrelation
    time, Geyer's initial monotone sequence), ess = draws / tau, mcse = sqrt(variance tau / draws), pairs (int64, the lag pairs
    the sequence used), truncated (bool: every pair was used, `lags` is too short), rhat (split-R-hat of the chain's two halves),
    all (n, C); columns: the C column names of the per-draw file."""

    def __init__(self, var, columns, parts):
        self.var, self.columns = var, list(columns)
        self.acov = parts["acov"]
        for name in _lib.ACF_FIELDS:
            setattr(self, name, parts[name])
        self.lags = int(self.acov.shape[2]) - 1

    def rows(self, idx):
        """The same object restricted to the windows idx."""
        return ChainAutocorr(self.var, self.columns, {k: getattr(self, k)[idx] for k in ("acov",) + _lib.ACF_FIELDS})


class ChainQuantiles:
    """Exact quantiles of one variable's draws over n windows (end dates), C columns and Q probabilities: value (n, C, Q) the
    quantile at probs[i] (numpy's / Julia's default definition), lo and hi (n, C, Q) the two draws that bracket it, g their
    weight (value = lo + g (hi - lo)); count and nan (n, C) int64 the draws ranked and the NaNs left out; columns: the C column
    names of the per-draw file."""

    def __init__(self, var, columns, probs, parts):
        self.var, self.columns, self.probs = var, list(columns), tuple(float(p) for p in probs)
        for name in _lib.ORD_FIELDS + ("count", "nan"):
            setattr(self, name, parts[name])

    def rows(self, idx):
        """The same object restricted to the windows idx."""
        return ChainQuantiles(self.var, self.columns, self.probs, {k: getattr(self, k)[idx] for k in _lib.ORD_FIELDS + ("count", "nan")})


class BatchResult:
    """Result of estimatewindows: per-window posterior summaries (+ optional draws)."""

    def __init__(self, opts, res, keep_draws):
        self.opts = opts
        self.summary = res["summary"]          # (W, 3K+K^2+2H)
        self.status = res["status"]
        self.kernel_ms = res.get("kernel_ms")
        self.corr = res.get("corr")            # (W, NC, NC) with corr=True: calccorr's matrix per window (corrnames)
        self.cdf = res.get("cdf")              # (W, n_h, G) with cdf_grid: calc_cdfs.jl's expectationsbar per window and horizon
        self.cdf_grid = res.get("cdf_grid")
        self.cdf_horizons = res.get("cdf_horizons")
        self.bias = res.get("bias")            # with bias_horizon: BiasMoments (uncerbias, totalbias, mean, cov) per window
        self.moments = res.get("moments")      # with moment_horizons: MixtureMoments, (W, n_h) arrays
        self.density = res.get("density")      # with density_vars: {var: ChainDensity}
        self.autocorr = res.get("autocorr")    # with acf_vars: {var: ChainAutocorr}
        self.quantiles = res.get("quantiles")  # with quantile_vars: {var: ChainQuantiles}
        self.ergodic = res.get("ergodic")      # with ergodic=True: the dict of _lib.unpack_ergodic, one row per window
        self.fan = res.get("fan")              # with fan_probs: the dict of _lib.unpack_fan plus probs, horizons, rounds
        self.scores = res.get("scores")        # with score_horizons: the dict of _lib.unpack_scores plus horizons, stride
        self._res = res if keep_draws else None

    def samples(self, w):
        if self._res is None:
            raise ValueError("draws were not kept (keep_draws=False)")
        o = self.opts[w]
        return _unpack(self._res, w, o.Nrun, o.D, len(o.horizons), enddate(o))


def _draw_vars(name, vars_):
    """The argument `name` of estimatewindows, names of draw arrays, as a tuple (None stays None)."""
    vars_ = None if vars_ is None else tuple(vars_)
    for var in vars_ or ():
        if var not in DENSITY_FILES:
            raise ValueError("%s: %r is none of %s" % (name, var, tuple(DENSITY_FILES)))
    return vars_


def estimatewindows(rawdata, dates, endIndices, startIndex=1, keep_draws=False, device=0, window_ids=None, corr=False,
                    cdf_grid=None, cdf_horizons=(0,), bias_horizon=None, moment_horizons=None, density_vars=None,
                    density_cuts=None, density_bins=64, density_trace=(0, 1), acf_vars=None, acf_lags=255, quantile_vars=None,
                    quantile_probs=(0.05, 0.5, 0.95), ergodic=False, fan_probs=None, fan_horizons=(0,), fan_rounds=0,
                    score_horizons=None, score_stride=0, **kwargs):
    """Batched estimatemodel over many expanding windows (one GPU call).

    Window w uses sampleRange = startIndex:endIndices[w], endIndex = endIndices[w]; the
    remaining keyword arguments are estopt's.  RNG stream ids default to the position
    in `endIndices`; pass window_ids to pin them (sharded runs).  corr=True also accumulates, on the device, the
    correlation matrix between each window's per-draw outputs (calccorr, src/Hmc.jl:1094-1163) -> BatchResult.corr.
    cdf_grid: grid points ys -> BatchResult.cdf (W, n_h, G), the draw mean of the regime mixture's normal CDF at every grid
    point (calc_cdfs.jl's expectationsbar; cdf_horizons: 0 = the end date, h > 0 = h steps ahead under pi_end A^h), computed on
    the device from the 5-digit-rounded draws (_lib.predictive_cdf_host); the draw arrays it needs are fetched for it and
    dropped again unless keep_draws.
    bias_horizon: h (upstream: 12) -> BatchResult.bias, the BiasMoments of bias_calcs.jl's calcbias per window (uncerbias,
    totalbias, mean, cov), computed on the device from the 5-digit-rounded draws (_lib.bias_moments_host); its draw arrays are
    fetched and dropped likewise.
    moment_horizons: horizons (0 = the end date, as skewness.jl; 12 as alt_forecasts.jl) -> BatchResult.moments, the
    MixtureMoments of the predictive regime mixture per window and horizon, computed on the device from the 5-digit-rounded
    draws (_lib.mixture_moments_host); its draw arrays are fetched and dropped likewise.
    density_vars: names among mu, sig2, pi_end, A, fcast -> BatchResult.density, {var: ChainDensity}: per window and column
    the binned counts of the chain prefixes density_cuts (default: the whole chain) on density_bins bins over the range of the
    draws, mean and variance of each prefix and the running mean density_trace = (length, stride) (mcplots.jl's plotchain and
    plotchainmean up to the drawing), computed on the device from the 5-digit-rounded draws (_lib.chain_density); the draw
    arrays are fetched and dropped likewise.
    acf_vars: names among mu, sig2, pi_end, A, fcast -> BatchResult.autocorr, {var: ChainAutocorr}: per window and column the
    autocovariances up to lag acf_lags, the integrated autocorrelation time, effective sample size, Monte-Carlo standard error
    and split-R-hat, computed on the device from the 5-digit-rounded draws (_lib.chain_autocorr); the draw arrays are fetched
    and dropped likewise.
    quantile_vars: names among mu, sig2, pi_end, A, fcast -> BatchResult.quantiles, {var: ChainQuantiles}: per window and column
    the exact quantiles at quantile_probs (at most 16) with the draws that bracket them, selected on the device from the
    5-digit-rounded draws (_lib.chain_quantiles); the draw arrays are fetched and dropped likewise.
    ergodic=True -> BatchResult.ergodic, the dict of _lib.unpack_ergodic: per window the mean and variance over the good draws
    of the stationary regime law, the expected durations and the long-run mean and variance of the series (the limit of
    pi_end A^h), computed on the device from the 5-digit-rounded draws (_lib.ergodic_moments); mu, sig2 and A are fetched and
    dropped likewise.
    fan_probs: at most 16 probabilities strictly inside (0, 1) -> BatchResult.fan, the dict of _lib.unpack_fan (quantile, lo, hi,
    Flo, Fhi (W, n_h, n_p), range, flag) with probs, horizons and rounds: per window, horizon of fan_horizons and probability
    the quantile of the predictive regime mixture -- the median, the bands of a fan chart, value-at-risk levels --, the CDF of
    cdf_grid inverted on the device by fan_rounds rounds of grid refinement (0: the default, 4) from the 5-digit-rounded draws
    (_lib.predictive_quantiles); its draw arrays are fetched and dropped likewise.
    score_horizons: horizons -> BatchResult.scores, the dict of _lib.unpack_scores (crps, e_abs, e_pair, pit, pdf, yreal, each
    (W, n_h)) with horizons and stride: per window and horizon h the continuous ranked probability score of the predictive
    regime mixture against the realised value y[end - 1 + h] of the series itself (NaN past its end: crps, e_abs, pit and pdf are
    then NaN), the probability integral transform and the predictive density there, computed on the device from the
    5-digit-rounded draws (_lib.predictive_scores) over every score_stride-th draw (0: thinned to at most 4 096 draws, 1: every
    draw, at a cost that grows with the square of Nrun * K); its draw arrays are fetched and dropped likewise."""
    if startIndex != 1:
        raise ValueError("windows must start at index 1 (see estopt)")
    acf_vars, density_vars = _draw_vars("acf_vars", acf_vars), _draw_vars("density_vars", density_vars)
    quantile_vars = _draw_vars("quantile_vars", quantile_vars)
    rawdata = np.asarray(rawdata, dtype=np.float64)
    opts = [estopt(rawdata, dates, sampleRange=range(1, int(e) + 1), endIndex=int(e), **kwargs) for e in endIndices]
    o0 = opts[0]
    for o in opts:
        _check_live_path(o)
        if len(o.signalRange):
            raise NotImplementedError("estimatewindows batches estimatemodel; use estimatesignals per window for signal runs")
    W = len(opts)
    Tw = np.array([len(o.sampleRange) for o in opts], dtype=np.int32)
    ld = int(Tw.max())
    Y = np.zeros((W, ld))
    yreal = np.zeros((W, len(o0.horizons)))
    for w, o in enumerate(opts):
        Y[w, :Tw[w]] = makey(o)
        yreal[w] = _yreal_row(rawdata, o.endIndex, o.horizons)
    want = keep_draws
    if not keep_draws:
        want = ()
        if cdf_grid is not None:
            want += ("mu", "sig2", "pi_end") + (("A",) if any(int(h) > 0 for h in cdf_horizons) else ())
        if bias_horizon is not None:
            want += ("mu", "pi_end") + (("A",) if int(bias_horizon) > 0 else ()) + (("fcast",) if len(o0.horizons) else ())
        if moment_horizons is not None:
            want += ("mu", "sig2", "pi_end") + (("A",) if any(int(h) > 0 for h in moment_horizons) else ())
        if density_vars is not None:
            want += tuple(density_vars)
        if acf_vars is not None:
            want += tuple(acf_vars)
        if quantile_vars is not None:
            want += tuple(quantile_vars)
        if ergodic:
            want += ("mu", "sig2", "A")
        if fan_probs is not None:
            want += ("mu", "sig2", "pi_end") + (("A",) if any(int(h) > 0 for h in fan_horizons) else ())
        if score_horizons is not None:
            want += ("mu", "sig2", "pi_end") + (("A",) if any(int(h) > 0 for h in score_horizons) else ())
        want = tuple(k for k in _lib.DRAW_KEYS if k in want) or False
    res = _lib.estimate_batch_host(Y, Tw, o0.D, o0.burnin, o0.Nrun, tuple(o0.horizons), yreal, seed=o0.seed,
                                   device=device, want_draws=want, window_ids=window_ids, want_corr=corr)
    if cdf_grid is not None:
        ys = np.ascontiguousarray(cdf_grid, dtype=np.float64).reshape(-1)
        hz = tuple(int(h) for h in cdf_horizons)
        res["cdf"] = _lib.predictive_cdf_host(res["mu"], res["sig2"], res["pi_end"], res.get("A") if any(h > 0 for h in hz) else None,
                                              ys, hz, device=device)
        res["cdf_grid"], res["cdf_horizons"] = ys, hz
    if bias_horizon is not None:
        h = int(bias_horizon)
        b = _lib.unpack_bias(_lib.bias_moments_host(res["mu"], res["pi_end"], res.get("A") if h > 0 else None,
                                                    res.get("fcast") if len(o0.horizons) else None, h, device=device), o0.D)
        res["bias"] = BiasMoments(h, b["uncerbias"], b["totalbias"], b["mean"], b["cov"])
    if moment_horizons is not None:
        hz = tuple(int(h) for h in moment_horizons)
        out = _lib.mixture_moments_host(res["mu"], res["sig2"], res["pi_end"], res.get("A") if any(h > 0 for h in hz) else None,
                                        hz, device=device)
        res["moments"] = MixtureMoments(hz, _lib.unpack_mixture_moments(out))
    if density_vars is not None:
        res["density"] = {}
        for var in density_vars:
            parts = _lib.chain_density(res[var], density_cuts, density_bins, None, density_trace, device=device)
            res["density"][var] = ChainDensity(var, _density_columns(o0, var), (o0.Nrun,) if density_cuts is None else density_cuts,
                                               density_trace[1], parts)
    if acf_vars is not None:
        res["autocorr"] = {var: ChainAutocorr(var, _density_columns(o0, var), _lib.chain_autocorr(res[var], acf_lags, device=device))
                           for var in acf_vars}
    if quantile_vars is not None:
        res["quantiles"] = {var: ChainQuantiles(var, _density_columns(o0, var), quantile_probs,
                                                _lib.chain_quantiles(res[var], quantile_probs, device=device))
                            for var in quantile_vars}
    if ergodic:
        res["ergodic"] = _lib.ergodic_moments(res["mu"], res["sig2"], res["A"], device=device)
    if fan_probs is not None:
        hz = tuple(int(h) for h in fan_horizons)
        res["fan"] = _lib.predictive_quantiles(res["mu"], res["sig2"], res["pi_end"], res.get("A") if any(h > 0 for h in hz) else None,
                                               fan_probs, hz, fan_rounds, device=device)
        res["fan"].update(probs=tuple(float(q) for q in fan_probs), horizons=hz, rounds=int(fan_rounds))
    if score_horizons is not None:
        hz = tuple(int(h) for h in score_horizons)
        yr = np.array([_yreal_row(rawdata, o.endIndex, hz) for o in opts]).reshape(W, len(hz)).T
        res["scores"] = _lib.predictive_scores(res["mu"], res["sig2"], res["pi_end"], res.get("A") if any(h > 0 for h in hz) else None,
                                               yr, hz, score_stride, device=device)
        res["scores"].update(horizons=hz, stride=int(score_stride))
    return BatchResult(opts, res, keep_draws)


# ----------------------------------------------------------------- CSV output --

def _fmt(x):
    """Float text in the style of the reference's committed CSVs (CSV.jl 0.5.16):
    shortest round-trip digits; integral values without a fraction; |x| < 1e-4 as
    <integer mantissa>e-<n> (e.g. 24e-11)."""
    x = float(x)
    if x != x:
        return "NaN"
    if x in (float("inf"), float("-inf")):
        return "Inf" if x > 0 else "-Inf"
    if x == int(x) and abs(x) < 1e15:
        return str(int(x))
    r = repr(x)
    if abs(x) < 1e-4:
        mant, exp = ("%r" % x).split("e") if "e" in r else (None, None)
        if mant is None:                       # repr chose positional notation (1e-4 > |x| >= 1e-5 never does)
            return r
        sign = "-" if mant.startswith("-") else ""
        mant = mant.lstrip("-")
        ip, _, fp = mant.partition(".")
        digits = (ip + fp).lstrip("0") or "0"
        e10 = int(exp) - len(fp)
        return "%s%se%d" % (sign, digits, e10)
    return r


def _header(opt, nfc):
    D = opt.D
    h1 = ["state_%d" % i for i in range(1, D + 1)]
    h2 = ["trans_%d_%d" % (i, j) for j in range(1, D + 1) for i in range(1, D + 1)]   # vec of [i,j] column-major (src/Hmc.jl:727)
    h3 = []
    for h in opt.horizons:
        h3 += ["forecast_%d" % h, "forecast_error_%d" % h]
    return h1, h2, h3[:nfc]


def basicsave(data, dates, fname, dataheader, precision=5, signal=None, signalids=None):
    """src/Hmc.jl:707-722: round to `precision` digits, date first; with signals a `signalid` column follows
    the date and `signal_i` columns (rounded to 5 digits) close the row."""
    data = np.asarray(data, dtype=np.float64)
    sc = 10.0 ** precision
    rounded = np.rint(data * sc) / sc
    header = ["date"] + list(dataheader)
    sig = None
    if signal is not None and np.asarray(signal).shape[1] > 0:
        sig = np.rint(np.asarray(signal, dtype=np.float64) * 1e5) / 1e5
        header += ["signal_%d" % (i + 1) for i in range(sig.shape[1])]
    if signalids is not None and len(signalids) > 0:
        header.insert(1, "signalid")
    with open(fname, "w") as f:
        f.write(",".join(header) + "\n")
        for i, (d, row) in enumerate(zip(dates, rounded)):
            cells = [str(d)]
            if sig is not None:                  # the reference only emits signalids together with signals (:715-717)
                cells.append(str(int(signalids[i])))
            cells += [_fmt(v) for v in row]
            if sig is not None:
                cells += [_fmt(v) for v in sig[i]]
            f.write(",".join(cells) + "\n")


def saveresults(samples, opt, dir, hassignals=False, native=True):
    """Five per-window CSVs with the reference's names and columns (src/Hmc.jl:724-748).
    Without signals the reference ignores `dir` and writes to data/output/<series>/ -- which is what its
    only caller passes (code/run_hmm.jl:116,120); with signals it writes under `dir` (:735-739).
    native=True (default) writes through the library's C writer (hmcg_save_results_csv: same bytes, ~100x the speed of
    the interpreted loop); native=False keeps the Python basicsave (used as the cross-check in the tests)."""
    os.makedirs(dir, exist_ok=True)
    h1, h2, h3 = _header(opt, samples.forecasts.shape[1])
    ed = enddate(opt)
    n = samples.μ.shape[0]
    if native:
        K = samples.μ.shape[1]
        H = samples.forecasts.shape[1] // 2
        res = dict(mu=samples.μ.T[None], sig2=samples.σ.T[None], pi_end=samples.πb[:, -1, :].T[None],
                   A=np.transpose(samples.A, (2, 1, 0))[None], fcast=samples.forecasts.T[None] if H else None)
        sv = None
        nsave = 0
        if hassignals and samples.signalvals is not None:
            ids = np.asarray(samples.signalids)
            ns = int(ids.max()) if len(ids) else 1
            per = n // ns
            sv = np.ascontiguousarray(np.asarray(samples.signalvals)[::per][None])      # (1, n_samples, nsave): one row per noise sample
            nsave = sv.shape[2]
        _lib.save_results_csv(dir, [ed], K, tuple(opt.horizons[:H]), res, sigvals=sv, nsave=nsave, n_threads=1)
        return
    kw = dict(signal=samples.signalvals, signalids=samples.signalids) if hassignals else {}
    basicsave(samples.μ, samples.obsdates, os.path.join(dir, "filtered_means_%s.csv" % ed), h1, **kw)
    basicsave(samples.σ, samples.obsdates, os.path.join(dir, "filtered_variances_%s.csv" % ed), h1, **kw)
    basicsave(samples.πb[:, -1, :], samples.obsdates, os.path.join(dir, "filtered_state_probs_%s.csv" % ed), h1, **kw)
    basicsave(samples.A.reshape(n, -1, order="F"), samples.obsdates,
              os.path.join(dir, "filtered_trans_probs_%s.csv" % ed), h2, **kw)
    basicsave(samples.forecasts, samples.obsdates, os.path.join(dir, "forecasts_%s.csv" % ed), h3, **kw)


SUMMARY_FILES = ("filtered_means", "filtered_variances", "filtered_state_probs", "filtered_trans_probs", "forecasts")


def write_summaries(summary, opts, dir, legacy_trans_header=False):
    """`*_summary.csv` files in runaggregate's layout (src/Hmc.jl:1025-1078): header
    `date,<col>_mean,...`, one row per end date in ascending date order.  `summary` is the
    (W, 3K+K^2+2H) block of on-device means of the 5-digit-rounded draws.
    legacy_trans_header reproduces the committed fixtures' trans_<j>_<i> naming
    (code/deprecated/Hmc.jl_08072019bak:711)."""
    os.makedirs(dir, exist_ok=True)
    o0 = opts[0]
    K, H = o0.D, len(o0.horizons)
    h1, h2, h3 = _header(o0, 2 * H)
    if legacy_trans_header:
        h2 = ["trans_%d_%d" % (j, i) for j in range(1, K + 1) for i in range(1, K + 1)]
    cols = [(0, K, h1), (K, 2 * K, h1), (2 * K, 3 * K, h1), (3 * K, 3 * K + K * K, h2),
            (3 * K + K * K, 3 * K + K * K + 2 * H, h3)]
    order = sorted(range(len(opts)), key=lambda w: enddate(opts[w]))
    paths = []
    for name, (a, b, hdr) in zip(SUMMARY_FILES, cols):
        p = os.path.join(dir, name + "_summary.csv")
        with open(p, "w") as f:
            f.write(",".join(["date"] + [h + "_mean" for h in hdr]) + "\n")
            for w in order:
                f.write(",".join([str(enddate(opts[w]))] + [_fmt(v) for v in summary[w, a:b]]) + "\n")
        paths.append(p)
    return paths


def write_signal_summaries(sample_summary, signalvals, opts, dir, legacy_trans_header=False):
    """The five `<var>_summary.csv` files runaggregate(datadir, var) (src/Hmc.jl:1053-1075) writes for a SIGNAL run -- header
    `date,signalid,<col>_mean...,signal_1_mean...`, one row per (date, noise sample), dates in ascending order as the per-draw
    files sort -- straight from the device's per-sample means (estimatesignalswindows(..., summaries=True)): the
    noiseSamples x signalNrun x 5 files of per-draw text per date are not needed.  The signal columns are constant within a
    sample; their "mean" is still taken as the file route takes it (the rounded value summed signalNrun times, divided), so
    that both routes print the same text (upstream's own fixture shows the effect: signal_1_mean = 12.408199999956814)."""
    os.makedirs(dir, exist_ok=True)
    o0 = opts[0]
    K, H = o0.D, len(o0.horizons)
    h1, h2, h3 = _header(o0, 2 * H)
    if legacy_trans_header:
        h2 = ["trans_%d_%d" % (j, i) for j in range(1, K + 1) for i in range(1, K + 1)]
    cols = [(0, K, h1), (K, 2 * K, h1), (2 * K, 3 * K, h1), (3 * K, 3 * K + K * K, h2),
            (3 * K + K * K, 3 * K + K * K + 2 * H, h3)]
    ns, nsave = sample_summary.shape[1], signalvals.shape[2]
    n = o0.signalNrun

    def const_mean(r):                                    # _seq_mean([r] * n) without the list
        if n <= 4096:
            acc = 0.0
            for _ in range(n):
                acc += r
            return acc / n
        return float(np.cumsum(np.full(n, r))[-1]) / n    # (cumsum adds in sequence)
    order = sorted(range(len(opts)), key=lambda w: enddate(opts[w]))
    paths = []
    for name, (a, b, hdr) in zip(SUMMARY_FILES, cols):
        p = os.path.join(dir, name + "_summary.csv")
        with open(p, "w") as f:
            f.write(",".join(["date", "signalid"] + [h + "_mean" for h in hdr] + ["signal_%d_mean" % (i + 1) for i in range(nsave)]) + "\n")
            for w in order:
                for smp in range(ns):
                    f.write(",".join([str(enddate(opts[w])), str(smp + 1)] + [_fmt(v) for v in sample_summary[w, smp, a:b]] +
                                     [_fmt(const_mean(float(np.rint(v * 1e5) / 1e5))) for v in signalvals[w, smp]]) + "\n")
        paths.append(p)
    return paths


# ------------------------------------------- aggregation over per-draw CSVs (host) --
# runaggregate / calcdispersion (src/Hmc.jl:1025-1092) work on the CSV files saveresults wrote, exactly as
# upstream: they are file-in / file-out and never touch the GPU.  For the estimatemodel path the on-device
# `summary` block (write_summaries above) gives the same numbers without the per-draw files.

def _read_csv(path):
    import csv
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def _seq_mean(vals):
    s = 0.0
    for v in vals:
        s += v
    return s / len(vals) if vals else float("nan")


def _seq_std(vals):
    """Statistics.std: corrected (n-1) two-pass sample standard deviation."""
    n = len(vals)
    if n < 2:
        return float("nan")
    m = _seq_mean(vals)
    s = 0.0
    for v in vals:
        s += (v - m) * (v - m)
    return math.sqrt(s / (n - 1))          # sqrt, not ** 0.5: pow() is not correctly rounded (3 of 456 lines differed in the last digit)


def _aggregate(header, rows, groups, funcs):
    """DataFrames.aggregate(df, groups, funcs): one row per group in order of first appearance; columns = groups,
    then for each function all non-group columns named <col>_<fname>."""
    gi = [header.index(g) for g in groups]
    vi = [i for i in range(len(header)) if i not in gi]
    order, buckets = [], {}
    for r in rows:
        key = tuple(r[i] for i in gi)
        if key not in buckets:
            buckets[key] = []
            order.append(key)
        buckets[key].append([float(r[i]) for i in vi])
    out_header = list(groups) + ["%s_%s" % (header[i], name) for name, _ in funcs for i in vi]
    out = []
    for key in order:
        cols = list(zip(*buckets[key]))
        out.append(list(key) + [_fmt(fn(list(c))) for _, fn in funcs for c in cols])
    return out_header, out


def _write_csv(path, header, rows):
    with open(path, "w") as f:
        f.write(",".join(header) + "\n")
        for r in rows:
            f.write(",".join(r) + "\n")


def runaggregate(datadir, var=None):
    """runaggregate(datadir) / runaggregate(datadir, var) (src/Hmc.jl:1025-1078): `<var>_summary.csv` = the mean of
    every column of each per-draw file `<var>_<date>.csv`, one row per date -- or per (date, signal) when the files
    carry signal columns.  As upstream, the one-argument form groups signal files by :signal_1 and the two-argument
    form by :signalid (the committed `forecasts_summary.csv` fixtures come from the latter)."""
    import glob
    if not os.path.isdir(datadir):
        raise ValueError("%s is not a valid directory" % datadir)
    first = sorted(glob.glob(os.path.join(datadir, "filtered_means*")))
    first = [f for f in first if "summary" not in f and "dispersion" not in f]
    hassignal = bool(first) and any("signal" in h for h in _read_csv(first[0])[0])
    groups = ["date"] if not hassignal else (["date", "signal_1"] if var is None else ["date", "signalid"])
    written = []
    for v in (SUMMARY_FILES_UPSTREAM_ORDER if var is None else (var,)):
        files = sorted(f for f in glob.glob(os.path.join(datadir, v + "*")) if "summary" not in f and "dispersion" not in f)
        if not files:
            continue
        out_header, out_rows = None, []
        for f in files:
            header, rows = _read_csv(f)
            h, r = _aggregate(header, rows, groups, [("mean", _seq_mean)])
            out_header = out_header or h
            out_rows += r
        path = os.path.join(datadir, v + "_summary.csv")
        _write_csv(path, out_header, out_rows)
        written.append(path)
    return written


SUMMARY_FILES_UPSTREAM_ORDER = ("filtered_means", "filtered_state_probs", "filtered_variances", "filtered_trans_probs", "forecasts")


def calcdispersion(datadir):
    """calcdispersion(datadir) (src/Hmc.jl:1080-1092): for each `<var>_summary.csv`, strip `_mean` from the column
    names and write mean and (n-1) standard deviation of every column per date to `<var>_dispersion.csv`
    (columns: date, all <col>_mean, then all <col>_std -- the signal id included, as upstream)."""
    if not os.path.isdir(datadir):
        raise ValueError("%s is not a valid directory" % datadir)
    written = []
    for v in SUMMARY_FILES_UPSTREAM_ORDER:
        src = os.path.join(datadir, v + "_summary.csv")
        if not os.path.exists(src):
            continue
        header, rows = _read_csv(src)
        header = [h.replace("_mean", "") for h in header]
        h, r = _aggregate(header, rows, ["date"], [("mean", _seq_mean), ("std", _seq_std)])
        path = os.path.join(datadir, v + "_dispersion.csv")
        _write_csv(path, h, r)
        written.append(path)
    return written


# ------------------------------------------------------------ correlation workbook --
# calccorr (src/Hmc.jl:1094-1163): per end date, the correlation matrix between the per-draw columns
# mu_1..K | sigma_1..K | pi_1..K | trans_* (file order) | forecast_<first horizon>, one workbook sheet per date plus, on
# the first sheet, the forecast's row of every date.  The matrices come either from the per-draw CSV files (as upstream:
# file in, file out, no GPU) or straight from the device (estimatewindows(..., corr=True): extras.corr, no per-draw file).

def corrnames(K, horizons):
    """Labels of a correlation matrix: what calccorr derives from the CSV headers (:1104,1109,1114,1122)."""
    return (["μ%d" % i for i in range(1, K + 1)] + ["σ%d" % i for i in range(1, K + 1)] + ["π%d" % i for i in range(1, K + 1)]
            + ["trans_%d_%d" % (i, j) for j in range(1, K + 1) for i in range(1, K + 1)] + ["forecast_%d" % horizons[0]])


def _xlsx_col(c):
    s = ""
    c += 1
    while c:
        c, r = divmod(c - 1, 26)
        s = chr(65 + r) + s
    return s


def _xlsx_sheet(cells):
    """cells: {(row, col): value} (0-based) -> worksheet XML; numbers as numeric cells, NaN / text as inline strings."""
    from xml.sax.saxutils import escape
    rows = {}
    for (r, c), v in cells.items():
        rows.setdefault(r, []).append((c, v))
    out = ['<?xml version="1.0" encoding="UTF-8" standalone="yes"?>\n'
           '<worksheet xmlns="http://schemas.openxmlformats.org/spreadsheetml/2006/main"><sheetData>']
    for r in sorted(rows):
        out.append('<row r="%d">' % (r + 1))
        for c, v in sorted(rows[r]):
            ref = "%s%d" % (_xlsx_col(c), r + 1)
            if isinstance(v, (int, float, np.floating)) and np.isfinite(v):
                out.append('<c r="%s"><v>%s</v></c>' % (ref, repr(float(v))))
            else:
                out.append('<c r="%s" t="inlineStr"><is><t>%s</t></is></c>' % (ref, escape(str(v))))
        out.append("</row>")
    out.append("</sheetData></worksheet>")
    return "".join(out)


def write_corr_workbook(path, dates, names, mats):
    """correlations.xlsx as calccorr lays it out (:1140-1161): sheet 1 ("Sheet1") = header row of the labels from B1 and
    one row per date (A: the date, B..: the LAST row of its matrix -- the forecast's correlations); then one sheet
    "yyyy_mm" per date holding the labelled matrix at A1 (corner cell: the date).  mats[i]: (NC, NC) array of dates[i]."""
    import zipfile
    names = list(names)
    sheets = [("Sheet1", {})]
    first = sheets[0][1]
    for c, nm in enumerate(names):
        first[(0, c + 1)] = nm
    for i, (d, m) in enumerate(zip(dates, mats)):
        d = str(d)
        m = np.asarray(m)
        first[(i + 1, 0)] = d
        for c in range(len(names)):
            first[(i + 1, c + 1)] = m[-1, c]
        cells = {(0, 0): d}
        for c, nm in enumerate(names):
            cells[(0, c + 1)] = nm
            cells[(c + 1, 0)] = nm
        for r in range(len(names)):
            for c in range(len(names)):
                cells[(r + 1, c + 1)] = m[r, c]
        sheets.append((d[0:4] + "_" + d[5:7], cells))
    ct = ['<?xml version="1.0" encoding="UTF-8" standalone="yes"?>\n<Types xmlns="http://schemas.openxmlformats.org/package/2006/content-types">'
          '<Default Extension="rels" ContentType="application/vnd.openxmlformats-package.relationships+xml"/>'
          '<Default Extension="xml" ContentType="application/xml"/>'
          '<Override PartName="/xl/workbook.xml" ContentType="application/vnd.openxmlformats-officedocument.spreadsheetml.sheet.main+xml"/>']
    wb = ['<?xml version="1.0" encoding="UTF-8" standalone="yes"?>\n<workbook xmlns="http://schemas.openxmlformats.org/spreadsheetml/2006/main" '
          'xmlns:r="http://schemas.openxmlformats.org/officeDocument/2006/relationships"><sheets>']
    rel = ['<?xml version="1.0" encoding="UTF-8" standalone="yes"?>\n<Relationships xmlns="http://schemas.openxmlformats.org/package/2006/relationships">']
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for i, (nm, cells) in enumerate(sheets, 1):
            ct.append('<Override PartName="/xl/worksheets/sheet%d.xml" ContentType="application/vnd.openxmlformats-officedocument.spreadsheetml.worksheet+xml"/>' % i)
            wb.append('<sheet name="%s" sheetId="%d" r:id="rId%d"/>' % (nm, i, i))
            rel.append('<Relationship Id="rId%d" Type="http://schemas.openxmlformats.org/officeDocument/2006/relationships/worksheet" Target="worksheets/sheet%d.xml"/>' % (i, i))
            z.writestr("xl/worksheets/sheet%d.xml" % i, _xlsx_sheet(cells))
        z.writestr("[Content_Types].xml", "".join(ct) + "</Types>")
        z.writestr("_rels/.rels", '<?xml version="1.0" encoding="UTF-8" standalone="yes"?>\n<Relationships xmlns="http://schemas.openxmlformats.org/package/2006/relationships">'
                   '<Relationship Id="rId1" Type="http://schemas.openxmlformats.org/officeDocument/2006/relationships/officeDocument" Target="xl/workbook.xml"/></Relationships>')
        z.writestr("xl/workbook.xml", "".join(wb) + "</sheets></workbook>")
        z.writestr("xl/_rels/workbook.xml.rels", "".join(rel) + "</Relationships>")
    return path


def _corr_from_files(datadir, date):
    """One date's labelled matrix from its five per-draw files, as calccorr reads them (:1100-1125)."""
    cols, names = [], []
    for stem, sym in (("filtered_means_", "μ"), ("filtered_variances_", "σ"), ("filtered_state_probs_", "π"),
                      ("filtered_trans_probs_", None), ("forecasts_", None)):
        header, rows = _read_csv(os.path.join(datadir, stem + date + ".csv"))
        data = np.array([[float(x) for x in r[1:]] for r in rows]).T
        hn = header[1:]
        if stem == "forecasts_":
            data, hn = data[:1], hn[:1]               # df4[!, [2]]: the first forecast column only (:1122)
        cols.append(data)
        names += [h.replace("state_", sym) if sym else h for h in hn]
    with np.errstate(invalid="ignore", divide="ignore"):
        return names, np.corrcoef(np.concatenate(cols))


def calccorr(datadir, startyear=1980, endyear=2018, startmonth=1, endmonth=2, result=None):
    """calccorr(datadir; startyear, endyear, startmonth, endmonth) (src/Hmc.jl:1094-1163): `correlations.xlsx` under
    datadir for the months from (startyear, startmonth) up to but excluding (endyear, endmonth).

    result=None: as upstream, every month's five per-draw files `filtered_*_<yyyy-mm>-01.csv` / `forecasts_<...>.csv` are
    read back and correlated on the host.  result = a BatchResult of estimatewindows(..., corr=True): the matrices were
    accumulated on the device while the draws were in HBM -- no per-draw file is read (or needs to exist); every month
    of the range must be one of the result's end dates.  Returns (path, dates, names, matrices)."""
    dates = []
    year, month = int(startyear), int(startmonth)
    while not (year == endyear and month == endmonth):
        dates.append("%04d-%02d-01" % (year, month))
        month += 1
        if month > 12:
            month, year = 1, year + 1
        if year > endyear + 1:
            raise ValueError("the month range never reaches (endyear, endmonth)")
    if not dates:
        raise ValueError("empty month range (upstream fails on data[1] here, src/Hmc.jl:1155)")
    mats, names = [], None
    if result is None:
        for d in dates:
            names, m = _corr_from_files(datadir, d)
            mats.append(m)
    else:
        if getattr(result, "corr", None) is None:
            raise ValueError("result carries no correlation matrices (estimatewindows(..., corr=True))")
        o0 = result.opts[0]
        names = corrnames(o0.D, o0.horizons)
        mats = [result.corr[w] for w in _rows_of(result, dates)]
    os.makedirs(datadir, exist_ok=True)
    path = write_corr_workbook(os.path.join(datadir, "correlations.xlsx"), dates, names, mats)
    return path, dates, names, mats


# ---------------------------------------------------------------- calc_cdfs.jl --

def _normcdf(z):
    """StatsFuns.normcdf: erfc(-z / sqrt 2) / 2, element by element."""
    erfc = np.frompyfunc(math.erfc, 1, 1)
    with np.errstate(invalid="ignore"):
        return (erfc(-np.asarray(z, dtype=np.float64) / math.sqrt(2.0)).astype(np.float64)) / 2.0


def _rows_of(result, dates):
    """The window of a BatchResult that ends on each of `dates`."""
    by_date = {str(enddate(o)): w for w, o in enumerate(result.opts)}
    for d in dates:
        if d not in by_date:
            raise ValueError("no window ends on %s" % d)
    return [by_date[d] for d in dates]


def _cells(datadir, stem, date):
    """One date's per-draw file `<stem>_<date>.csv` without its date column: (column names, cells (n, C))."""
    header, rows = _read_csv(os.path.join(datadir, "%s_%s.csv" % (stem, date)))
    return header[1:], np.array([[float(x) for x in r[1:]] for r in rows])


def _mixture_cells(datadir, date, horizons):
    """means, vars_, pis (n, K) and, with a horizon > 0, trans (n, K * K) of one date: the files the mixture statistics read."""
    means, vars_, pis = (_cells(datadir, stem, date)[1] for stem in ("filtered_means", "filtered_variances", "filtered_state_probs"))
    return means, vars_, pis, (_cells(datadir, "filtered_trans_probs", date)[1] if any(h > 0 for h in horizons) else None)


def _omega(pis, trans, h):
    """pis * A^h per draw: pis (n, K), trans (n, K * K) in the file's column order (trans_i_j, i fastest; not read at h = 0).
    One product at a time with i ascending, the library's expression (HMCG_OMEGA_STEP), so the file routes keep its bits."""
    n, K = pis.shape
    w = np.array(pis, dtype=np.float64)
    if h > 0:
        A = trans.reshape(n, K, K).transpose(0, 2, 1)                                       # A[d, i, j]
    for _ in range(h):
        nw = w[:, 0, None] * A[:, 0, :]
        for i in range(1, K):
            nw = nw + w[:, i, None] * A[:, i, :]
        w = nw
    return w


def _cdfs_from_files(datadir, date, ys, horizons):
    """One date's expectationsbar (n_h, G) from its per-draw files, as calc_cdfs.jl:33-41 computes it on the host."""
    means, vars_, pis, trans = _mixture_cells(datadir, date, horizons)
    return _cdfs_from_cells(means, vars_, pis, trans, ys, horizons)


def _cdfs_from_cells(means, vars_, pis, trans, ys, horizons):
    """expectationsbar (n_h, G) from the cells of one date's files: (n, K) each, trans (n, K * K) in the file's column order."""
    n, K = means.shape
    with np.errstate(invalid="ignore", divide="ignore"):
        z = (ys[None, :, None] - means[:, None, :]) / np.sqrt(vars_)[:, None, :]           # (n, G, K)
    phi = _normcdf(z)
    out = np.empty((len(horizons), len(ys)))
    for j, h in enumerate(horizons):
        w = _omega(pis, trans, h)                                                           # S0 * A^h
        f = w[:, None, 0] * phi[:, :, 0]
        for k in range(1, K):
            f = f + w[:, None, k] * phi[:, :, k]
        out[j] = np.mean(f, axis=0)
    return out


def finverse(p):
    """quantile.(Normal(), p) (calc_cdfs.jl:42): 0 -> -Inf, 1 -> +Inf, NaN (or a value outside [0, 1]) -> NaN."""
    import statistics
    nd = statistics.NormalDist()

    def one(x):
        x = float(x)
        if x == 0.0:
            return -math.inf
        if x == 1.0:
            return math.inf
        if not 0.0 < x < 1.0:
            return math.nan
        return nd.inv_cdf(x)
    with np.errstate(invalid="ignore"):
        return np.frompyfunc(one, 1, 1)(np.asarray(p, dtype=np.float64)).astype(np.float64)


def calccdfs(datadir, dates, ys=np.arange(-5, 15.25, .25), horizons=(0,), result=None):
    """code/hassan_cdfs/calc_cdfs.jl:31-42 without the plots: for every end date the draw mean of
    F_i(y) = sum_k pi_i[k] Phi((y - mu_i[k]) / sqrt(var_i[k])) on the grid ys (`expectationsbar`) and its image under the normal
    quantile (`finverse`).  horizons: 0 = the end date, as upstream; h > 0 weights the states by pi_i A_i^h instead.

    result=None: as upstream, every date's `filtered_means_`, `filtered_variances_`, `filtered_state_probs_<date>.csv` (and
    `filtered_trans_probs_<date>.csv` with a horizon > 0) are read back and evaluated on the host in numpy; no GPU is touched.
    result = a BatchResult of estimatewindows(..., cdf_grid=ys, cdf_horizons=horizons): the means were taken on the device
    from the rounded draws; every date must be one of the result's end dates.
    Returns (dates, ys, expectationsbar (n_dates, n_h, G), finverse of the same shape)."""
    dates = [str(d) for d in dates]
    ys = np.ascontiguousarray(ys, dtype=np.float64).reshape(-1)
    horizons = tuple(int(h) for h in horizons)
    if result is None:
        bar = np.array([_cdfs_from_files(datadir, d, ys, horizons) for d in dates]).reshape(len(dates), len(horizons), len(ys))
    else:
        if getattr(result, "cdf", None) is None:
            raise ValueError("result carries no predictive CDFs (estimatewindows(..., cdf_grid=ys))")
        if not np.array_equal(result.cdf_grid, ys) or tuple(result.cdf_horizons) != horizons:
            raise ValueError("result was computed on another grid or other horizons")
        bar = np.array([result.cdf[w] for w in _rows_of(result, dates)]).reshape(len(dates), len(horizons), len(ys))
    return dates, ys, bar, finverse(bar)


def write_cdfs(path, dates, ys, horizons, expectationsbar):
    """One CSV `date,horizon,y,cdf,finverse` with a row per (date, horizon, grid point), float text as in the other files (_fmt).
    Upstream writes only plots of these numbers (calc_cdfs.jl:44), so this layout is this project's own."""
    bar = np.asarray(expectationsbar, dtype=np.float64)
    fin = finverse(bar)
    rows = [[str(d), str(int(h)), _fmt(y), _fmt(bar[i, j, g]), _fmt(fin[i, j, g])]
            for i, d in enumerate(dates) for j, h in enumerate(horizons) for g, y in enumerate(ys)]
    _write_csv(path, ["date", "horizon", "y", "cdf", "finverse"], rows)
    return path


# --------------------------------------------------------------- bias_calcs.jl --

def _bias_from_cells(means, states, trans, ferr, horizon):
    """calcbias (bias_calcs.jl:40-53) on the cells of one date's files: means, states (n, K), trans (n, K * K) in the file's
    column order (trans_i_j, i fastest), ferr (n,) the forecast_error column of the first horizon or None.  Returns
    (uncbias, totalbias, mean (2K,), cov (2K, 2K)), the last two in the order futstate | means."""
    n, K = means.shape
    fut = _omega(states, trans, horizon)                                                    # states' * A^h
    v = np.hstack([fut, means])
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = v.mean(axis=0)
        dv = v - mean
        covv = dv.T @ dv / (n - 1.0)                                                        # cov(hcat(futstate, means))
        nab = np.hstack([means, fut]).mean(axis=0)                                          # mean(hcat(means, futstate), dims=1)
        unc = float(nab @ covv @ nab)                                                       # upstream's index swap, kept
        tot = float(np.mean(ferr)) if ferr is not None else math.nan
    return unc, tot, mean, covv


def _bias_from_files(datadir, date, horizon):
    means, states, trans, fc = (_cells(datadir, stem, date)[1]
                                for stem in ("filtered_means", "filtered_state_probs", "filtered_trans_probs", "forecasts"))
    return _bias_from_cells(means, states, trans, fc[:, 1], horizon)                        # forecasts[:, 3]: date, forecast, error


def calcbias(datadir, dates, horizon=12, result=None):
    """code/hassan_cdfs/bias_calcs.jl:40-53 without the plot: per end date `uncerbias` = nab * covv * nab' with
    covv = cov(hcat(futstate, means)), nab = mean(hcat(means, futstate)), futstate = states * trans^horizon per draw -- the two
    column orders differ upstream and are kept -- and `totalbias` = the mean of the first horizon's forecast_error column.

    result=None: as upstream, every date's `filtered_means_`, `filtered_state_probs_`, `filtered_trans_probs_` and
    `forecasts_<date>.csv` are read back and evaluated on the host in numpy; no GPU is touched.
    result = a BatchResult of estimatewindows(..., bias_horizon=horizon): the moments were taken on the device from the rounded
    draws; every date must be one of the result's end dates.
    Returns (dates, uncerbias (n_dates,), totalbias (n_dates,), mean (n_dates, 2K), cov (n_dates, 2K, 2K)); mean and cov are
    those of [futstate | means]."""
    dates = [str(d) for d in dates]
    horizon = int(horizon)
    if result is None:
        rows = [_bias_from_files(datadir, d, horizon) for d in dates]
        unc, tot = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
        mean, cov = np.array([r[2] for r in rows]), np.array([r[3] for r in rows])
    else:
        b = getattr(result, "bias", None)
        if b is None:
            raise ValueError("result carries no bias moments (estimatewindows(..., bias_horizon=h))")
        if b.horizon != horizon:
            raise ValueError("result was computed for another horizon")
        idx = _rows_of(result, dates)
        unc, tot, mean, cov = b.uncerbias[idx], b.totalbias[idx], b.mean[idx], b.cov[idx]
    return dates, unc, tot, mean, cov


def write_biases(path, dates, uncerbias, totalbias):
    """One CSV `date,uncerbias,totalbias` with a row per end date, float text as in the other files (_fmt).  Upstream only
    plots these numbers (bias_calcs.jl:63-64), so this layout is this project's own."""
    rows = [[str(d), _fmt(u), _fmt(t)] for d, u, t in zip(dates, uncerbias, totalbias)]
    _write_csv(path, ["date", "uncerbias", "totalbias"], rows)
    return path


# ------------------------------------------------ skewness.jl, alt_forecasts.jl --

def _moments_from_cells(means, vars_, pis, trans, horizons):
    """The (n_h, 8) block of include/hmcg.h's table from the cells of one date's files: (n, K) each, trans (n, K * K) in the
    file's column order.  The library's algebra in numpy: per-draw closed-form moments about the pivot c = the mixture mean of
    draw 0, summed over the draws."""
    n, K = means.shape
    out = np.empty((len(horizons), _lib.MIX_STRIDE))
    for j, h in enumerate(horizons):
        w = _omega(pis, trans, h)                                                           # pi_end * A^h
        with np.errstate(invalid="ignore", divide="ignore"):
            s = w.sum(axis=1)
            c = (w[0] * means[0]).sum() / s[0]
            d = means - c
            d2 = d * d
            P = [s.sum(), (w * d).sum(), (w * (d2 + vars_)).sum(), (w * d * (d2 + 3.0 * vars_)).sum(),
                 (w * (d2 * d2 + 6.0 * d2 * vars_ + 3.0 * vars_ * vars_)).sum()]
            a = (w * d).sum(axis=1) / s
            e = d - a[:, None]
            var_d = (w * (e * e + vars_)).sum(axis=1) / s
            skew_d = (w * e * (e * e + 3.0 * vars_)).sum(axis=1) / s / (var_d * np.sqrt(var_d))
            b = a - a[0]
            m1, m2, m3, m4 = (p / P[0] for p in P[1:])
            var = m2 - m1 * m1
            out[j] = [c + m1, var, (m3 - 3.0 * m1 * m2 + 2.0 * m1 ** 3) / (var * np.sqrt(var)),
                      (m4 - 4.0 * m1 * m3 + 6.0 * m1 * m1 * m2 - 3.0 * m1 ** 4) / (var * var) - 3.0,
                      var_d.sum() / n, (b * b).sum() / n - (b.sum() / n) ** 2, skew_d.sum() / n, P[0] / n]
    return out


def _moments_from_files(datadir, date, horizons):
    return _moments_from_cells(*_mixture_cells(datadir, date, horizons), horizons)


def calcmoments(datadir, dates, horizons=(0,), result=None):
    """What code/skewness.jl and code/alt_forecasts.jl ask of the posterior-summary rows, asked of the draws: per end date and
    horizon h the moments of the predictive law y_{T+h} ~ sum_k omega_k N(mu_k, sig2_k), omega = pi_end A^h, pooled over the
    draws in closed form -- mean (the proper forecast alt_forecasts.jl sets its plug-in against), variance, skewness (what
    skewness.jl samples for, with the parameter uncertainty in), excess kurtosis -- and the split a plug-in hides: `within`
    (mean per-draw variance), `between` (variance over the draws of the per-draw mean), `draw_skewness`, `weight`.

    result=None: every date's `filtered_means_`, `filtered_variances_`, `filtered_state_probs_<date>.csv` (and
    `filtered_trans_probs_<date>.csv` with a horizon > 0) are read back and evaluated on the host in numpy; no GPU is touched.
    result = a BatchResult of estimatewindows(..., moment_horizons=horizons): the sums were taken on the device from the
    rounded draws; every date must be one of the result's end dates.
    Returns (dates, moments): a dict of (n_dates, n_h) arrays under the names of _lib.MIX_FIELDS."""
    dates = [str(d) for d in dates]
    horizons = tuple(int(h) for h in horizons)
    if result is None:
        block = np.array([_moments_from_files(datadir, d, horizons) for d in dates]).reshape(len(dates), len(horizons), _lib.MIX_STRIDE)
        return dates, _lib.unpack_mixture_moments(block)
    m = getattr(result, "moments", None)
    if m is None:
        raise ValueError("result carries no mixture moments (estimatewindows(..., moment_horizons=hs))")
    if m.horizons != horizons:
        raise ValueError("result was computed for other horizons")
    idx = _rows_of(result, dates)
    return dates, {name: getattr(m, name)[idx] for name in _lib.MIX_FIELDS}


def _summary_rows(datadir, stem):
    """`<stem>_summary.csv` of runaggregate: (header, dates, cells (n_dates, n_columns))."""
    header, rows = _read_csv(os.path.join(datadir, stem + "_summary.csv"))
    return header, [r[0] for r in rows], np.array([[float(x) for x in r[1:]] for r in rows])


def calcskewness(datadir, date=None):
    """code/skewness.jl:22-43 in closed form.  Upstream builds the mixture sum_k p_k N(mu_k, sqrt(var_k)) from the row of the
    latest date in `filtered_means_`, `filtered_variances_` and `filtered_state_probs_summary.csv` (p normalised to sum 1, :33),
    draws 10 000 000 variates and averages ((x - mean(f)) / std(f))^3; that average estimates
    sum_k p_k e_k (e_k^2 + 3 var_k) / std^3, e_k = mu_k - mean, which is returned here.  date: another row's date (default: the
    latest, as upstream).  Returns (date, mean, std, skewness)."""
    _, dates, mu = _summary_rows(datadir, "filtered_means")
    _, dv, var = _summary_rows(datadir, "filtered_variances")
    _, dp, p = _summary_rows(datadir, "filtered_state_probs")
    date = max(dates) if date is None else str(date)
    mu, var, p = mu[dates.index(date)], var[dv.index(date)], p[dp.index(date)]
    p = p / p.sum()
    mean = float(np.dot(p, mu))
    e = mu - mean
    v = float(np.dot(p, e * e + var))
    return date, mean, math.sqrt(v), float(np.dot(p, e * (e * e + 3.0 * var))) / (v * math.sqrt(v))


def altforecasts(datadir, horizon=12):
    """code/alt_forecasts.jl:23-38: per row of the summary files the plug-in forecast `forecast_post` = dot(pi' * A^12, mu) from
    the posterior means of `filtered_means_`, `filtered_state_probs_` and `filtered_trans_probs_summary.csv` -- A is
    reshape(row, K, K), column-major, whatever the header calls the columns (:33) -- beside `forecast_proper`, the
    `forecast_12_mean` column of `forecasts_summary.csv` (the draw mean of the forecast), row by row as upstream pairs them.
    Returns (dates, forecast_post, forecast_proper)."""
    _, dates, mu = _summary_rows(datadir, "filtered_means")
    _, _, pis = _summary_rows(datadir, "filtered_state_probs")
    _, _, trans = _summary_rows(datadir, "filtered_trans_probs")
    hf, _, fc = _summary_rows(datadir, "forecasts")
    n, K = mu.shape
    A = trans.reshape(n, K, K).transpose(0, 2, 1)                                           # A[r, i, j] = row[i + K j]
    w = pis.copy()
    for _ in range(int(horizon)):
        nw = w[:, 0, None] * A[:, 0, :]
        for i in range(1, K):
            nw = nw + w[:, i, None] * A[:, i, :]
        w = nw
    post = w[:, 0] * mu[:, 0]
    for k in range(1, K):
        post = post + w[:, k] * mu[:, k]
    return dates, post, fc[:, hf.index("forecast_%d_mean" % int(horizon)) - 1]


def write_forecast_comparison(path, dates, forecast_post, forecast_proper):
    """alt_forecasts.jl:28,39: `date,forecast_post,forecast_proper`, one row per end date, float text as in the other files (_fmt)."""
    rows = [[str(d), _fmt(a), _fmt(b)] for d, a, b in zip(dates, forecast_post, forecast_proper)]
    _write_csv(path, ["date", "forecast_post", "forecast_proper"], rows)
    return path


# ------------------------------------------- plots/mcplots.jl, timeseriesplots.jl --

def _density_columns(opt, var):
    """The column names of the per-draw file of `var` (saveresults)."""
    h1, h2, h3 = _header(opt, 2 * len(opt.horizons))
    return {"A": h2, "fcast": h3}.get(var, h1)


def _bin_slots(v, lo, hi, bins):
    """The bin rule of include/hmcg.h on a 1-D array: the bin per value, -1 below, -2 above, -3 NaN."""
    isn = np.isnan(v)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        below = ~isn & (bool(np.isnan(lo) or np.isnan(hi)) | (v < lo))
        above = ~isn & ~below & (v > hi)
        slot = np.zeros(v.shape, dtype=np.int64)
        if hi > lo:
            scale = np.float64(bins) / (np.float64(hi) - np.float64(lo))
            t = np.floor((v - np.float64(lo)) * scale)
            slot = np.clip(np.where(np.isnan(t), 0.0, t), 0.0, float(bins - 1)).astype(np.int64)
    slot[below], slot[above], slot[isn] = -1, -2, -3
    return slot


def _density_from_cells(cells, cuts, bins, lo_hi, trace):
    """The outputs of hmcg_chain_density for one date from the cells (n, C) of its per-draw file, in numpy fp64 with the
    library's algebra (sums about the pivot p = row 0).  Returns the parts of _lib.DENS_FIELDS without the window axis."""
    n, Cn = cells.shape
    nc, tl, ts = len(cuts), int(trace[0]), int(trace[1])
    out = {"counts": np.zeros((Cn, nc, bins), dtype=np.int64), "below": np.zeros((Cn, nc), dtype=np.int64),
           "above": np.zeros((Cn, nc), dtype=np.int64), "nan": np.zeros((Cn, nc), dtype=np.int64), "range": np.empty((Cn, 2)),
           "mean": np.empty((Cn, nc)), "variance": np.empty((Cn, nc)), "trace": np.empty((Cn, tl))}
    idx = (np.arange(tl) + 1) * ts - 1
    for c in range(Cn):
        v = cells[:, c]
        fin = v[np.isfinite(v)]
        if lo_hi is not None:
            lo, hi = lo_hi[c]
        elif fin.size:
            lo, hi = fin.min(), fin.max()
        else:
            lo = hi = np.nan
        out["range"][c] = lo, hi
        slot = _bin_slots(v, lo, hi, bins)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            a = v - v[0]
            for j, cut in enumerate(cuts):
                s = slot[:cut]
                out["counts"][c, j] = np.bincount(s[s >= 0], minlength=bins)
                out["below"][c, j], out["above"][c, j], out["nan"][c, j] = (s == -1).sum(), (s == -2).sum(), (s == -3).sum()
                S1, S2, m = a[:cut].sum(), (a[:cut] * a[:cut]).sum(), float(cut)
                out["mean"][c, j] = v[0] + S1 / m
                out["variance"][c, j] = (S2 - S1 * S1 / m) / (m - 1.0)
            out["trace"][c] = v[0] + np.cumsum(a)[idx] / (idx + 1.0)
    return out


def calcchain(datadir, dates, var="mu", cuts=None, bins=64, lo_hi=None, trace=(0, 1), result=None):
    """plots/mcplots.jl:24-38 (plotchain), :47-63 (plotchainmean) and plots/timeseriesplots.jl:83-142 (plot_mean / plot_var) up
    to the drawing: per end date and column of one variable's per-draw file the binned counts of the chain prefixes 1:cuts[j]
    (mcplots.jl: 100000, 150000, 200000, 250000; default: the whole chain), mean and variance of each prefix, and the running
    mean after (i + 1) * trace[1] draws, i < trace[0] (plotchainmean: (10000, 1)).  var: mu, sig2, pi_end, A or fcast.

    result=None: every date's `filtered_means_<date>.csv` (`filtered_variances_`, `filtered_state_probs_`,
    `filtered_trans_probs_`, `forecasts_` for the other variables) is read back as the plot scripts read it and evaluated on the
    host in numpy; no GPU is touched.  lo_hi: (n_dates, C, 2) bin ranges (default: the range of each column's finite cells).
    result = a BatchResult of estimatewindows(..., density_vars=(var, ...)): the counts and sums were taken on the device from
    the rounded draws; every date must be one of the result's end dates, and cuts / bins / trace must be the result's.
    Returns (dates, ChainDensity)."""
    dates = [str(d) for d in dates]
    if var not in DENSITY_FILES:
        raise ValueError("var must be one of %s" % (tuple(DENSITY_FILES),))
    if result is not None:
        d = getattr(result, "density", None)
        if d is None or var not in d:
            raise ValueError("result carries no chain density of %s (estimatewindows(..., density_vars=(%r,)))" % (var, var))
        d = d[var]
        if (cuts is not None and tuple(int(c) for c in cuts) != d.cuts) or int(bins) != d.bins or \
                (int(trace[0]), int(trace[1])) != (d.trace.shape[2], d.trace_stride):
            raise ValueError("result was computed for other cuts, bins or trace")
        return dates, d.rows(_rows_of(result, dates))
    parts, columns, used = [], None, None
    for i, date in enumerate(dates):
        columns, cells = _cells(datadir, DENSITY_FILES[var], date)
        ct = (cells.shape[0],) if cuts is None else tuple(int(c) for c in cuts)
        if used is not None and ct != used:
            raise ValueError("the dates' files differ in length: give cuts")
        used = ct
        if any(c < 1 or c > cells.shape[0] for c in ct) or int(trace[0]) * int(trace[1]) > cells.shape[0]:
            raise ValueError("cuts or trace reach beyond the %d draws of %s" % (cells.shape[0], date))
        parts.append(_density_from_cells(cells, ct, int(bins), None if lo_hi is None else np.asarray(lo_hi, dtype=np.float64)[i], trace))
    return dates, ChainDensity(var, columns, used, trace[1], {k: np.array([q[k] for q in parts]) for k in _lib.DENS_FIELDS})


def chainquantiles(density, qs):
    """Credible limits at bin resolution: per window, column and prefix, for each q in qs the bin that holds the order
    statistic ceil(q * n) (1 <= . <= n) of the n non-NaN draws of the prefix -- exact by construction, since the counts say how
    many draws lie below each bin.  Returns a dict of (n, C, n_cuts, len(qs)) arrays: bin (-1: below lo, bins: above hi), lo and
    hi, the bin's edges range_lo + b * (range_hi - range_lo) / bins (-inf / +inf on the open side of below / above; NaN with no
    draw to rank)."""
    qs = np.atleast_1d(np.asarray(qs, dtype=np.float64))
    B = density.bins
    full = np.concatenate([density.below[..., None], density.counts, density.above[..., None]], axis=3)      # order: below, bins, above
    cum = np.cumsum(full, axis=3)
    n = cum[..., -1]
    shape = n.shape + (qs.size,)
    out = {"bin": np.empty(shape, dtype=np.int64), "lo": np.empty(shape), "hi": np.empty(shape)}
    lo, hi = density.range[..., 0][:, :, None], density.range[..., 1][:, :, None]
    with np.errstate(invalid="ignore"):
        edges = lo[..., None] + np.arange(B + 1) * ((hi - lo) / B)[..., None]                                # (n, C, 1, B + 1)
    edges = np.broadcast_to(edges, n.shape + (B + 1,))
    for i, q in enumerate(qs):
        k = np.clip(np.ceil(q * n), 1, np.maximum(n, 1)).astype(np.int64)
        b = (cum < k[..., None]).sum(axis=3) - 1                      # first slot whose running count reaches k, as a bin index
        b = np.minimum(b, B)
        inside = np.clip(b, 0, B - 1)
        el = np.take_along_axis(edges, inside[..., None], axis=3)[..., 0]
        eh = np.take_along_axis(edges, inside[..., None] + 1, axis=3)[..., 0]
        l = np.where(b < 0, -np.inf, np.where(b >= B, np.broadcast_to(hi, b.shape), el))
        h = np.where(b < 0, np.broadcast_to(lo, b.shape), np.where(b >= B, np.inf, eh))
        none = n == 0
        out["bin"][..., i] = np.where(none, -1, b)
        out["lo"][..., i] = np.where(none, np.nan, l)
        out["hi"][..., i] = np.where(none, np.nan, h)
    return out


def chaindensity(density, points=None, bandwidth=None):
    """What Gadfly's Geom.density draws in plotchain / plot_mean / plot_var, from the binned counts: the Gaussian kernel
    estimate f(x) = sum_b counts_b N(x; centre_b, h) / sum_b counts_b over the in-range draws, a discrete convolution of the
    histogram with the kernel sampled at the bin spacing when points is None (the points are then the bin centres).
    h is Silverman's rule 0.9 min(sd, IQR / 1.34) n^(-1/5) with sd from the prefix's variance and IQR from the centres of the
    bins that hold the quartiles (chainquantiles); where that is 0 or NaN, the bin width.  bandwidth: a number that overrides it.
    Upstream's KernelDensity.jl picks its own grid (2048 points on a padded range) and bandwidth; neither is pinned here, so the
    curves agree in shape, not point for point.
    Returns a dict: x (n, C, P) points, density (n, C, n_cuts, P), bandwidth (n, C, n_cuts)."""
    B = density.bins
    lo, hi = density.range[..., 0], density.range[..., 1]
    width = (hi - lo) / B
    centres = lo[..., None] + (np.arange(B) + 0.5) * width[..., None]                    # (n, C, B)
    n_in = density.counts.sum(axis=3).astype(np.float64)
    q = chainquantiles(density, (0.25, 0.75))
    with np.errstate(invalid="ignore", divide="ignore"):
        iqr = ((np.clip(q["bin"][..., 1], 0, B - 1) - np.clip(q["bin"][..., 0], 0, B - 1)) * width[..., None]).astype(np.float64)
        sd = np.sqrt(density.variance)
        spread = np.where(iqr > 0, np.minimum(sd, iqr / 1.34), sd)
        h = 0.9 * spread * n_in ** -0.2
        h = np.where(np.isfinite(h) & (h > 0), h, np.broadcast_to(width[..., None], h.shape))
    if bandwidth is not None:
        h = np.full(h.shape, float(bandwidth))
    nW, Cn, nc = h.shape
    if points is None:
        x = centres
    else:
        x = np.broadcast_to(np.asarray(points, dtype=np.float64), (nW, Cn, np.size(points))).copy()
    dens = np.full((nW, Cn, nc, x.shape[2]), np.nan)
    for w in range(nW):
        for c in range(Cn):
            for j in range(nc):
                hh, tot = h[w, c, j], n_in[w, c, j]
                if not (tot > 0 and np.isfinite(hh) and hh > 0):
                    continue
                cnt = density.counts[w, c, j].astype(np.float64)
                if points is None:
                    off = np.arange(-(B - 1), B) * width[w, c]                          # the kernel at the bin spacing
                    ker = np.exp(-0.5 * (off / hh) ** 2) / (hh * math.sqrt(2.0 * math.pi))
                    dens[w, c, j] = np.convolve(cnt, ker)[B - 1:2 * B - 1] / tot
                else:
                    z = (x[w, c][:, None] - centres[w, c][None, :]) / hh
                    dens[w, c, j] = (np.exp(-0.5 * z * z) @ cnt) / (hh * math.sqrt(2.0 * math.pi) * tot)
    return {"x": x, "density": dens, "bandwidth": h}


def write_chain_density(path, dates, density):
    """`date,column,cut,bin_lo,bin_hi,count,density`: one row per end date, column, prefix and bin -- the bin's edges, its count
    and the kernel estimate at its centre (chaindensity).  Our layout: upstream draws the figure and writes no file."""
    kde = chaindensity(density)["density"]
    B = density.bins
    rows = []
    for w, d in enumerate(dates):
        for c, name in enumerate(density.columns):
            lo, hi = density.range[w, c]
            for j, cut in enumerate(density.cuts):
                for b in range(B):
                    rows.append([str(d), name, str(cut), _fmt(lo + b * ((hi - lo) / B)), _fmt(lo + (b + 1) * ((hi - lo) / B)),
                                 str(int(density.counts[w, c, j, b])), _fmt(kde[w, c, j, b])])
    _write_csv(path, ["date", "column", "cut", "bin_lo", "bin_hi", "count", "density"], rows)
    return path


def write_chain_trace(path, dates, density):
    """`date,column,draws,mean`: the running mean of plotchainmean, one row per end date, column and trace point."""
    rows = []
    for w, d in enumerate(dates):
        for c, name in enumerate(density.columns):
            for i in range(density.trace.shape[2]):
                rows.append([str(d), name, str((i + 1) * density.trace_stride), _fmt(density.trace[w, c, i])])
    _write_csv(path, ["date", "column", "draws", "mean"], rows)
    return path


# ------------------------------------------- autocorrelation, effective sample size, split-R-hat --

def _geyer(acov, variance, n):
    """The derived block of include/hmcg.h for one column in fp64: tau, ess, mcse, pairs, truncated."""
    nan, n = np.float64(np.nan), np.float64(n)
    a0 = np.float64(acov[0])
    if not (a0 > 0.0):
        return nan, nan, nan, 0, False
    npairs, k = len(acov) // 2, 0
    tau, prev = np.float64(-1.0), np.float64(np.inf)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        while k < npairs:
            P = np.float64(acov[2 * k]) / a0 + np.float64(acov[2 * k + 1]) / a0
            if not (P > 0.0):
                break
            P = min(P, prev)
            tau = tau + np.float64(2.0) * P
            prev = P
            k += 1
        if k == 0:
            tau = nan
        return tau, n / tau, np.sqrt((np.float64(variance) * tau) / n), k, k == npairs


def _autocorr_from_cells(cells, lags):
    """The outputs of hmcg_chain_autocorr for one date from the cells (n, C) of its per-draw file, in numpy fp64 with the
    library's algebra (sums about the pivot p = row 0).  Returns the parts of a ChainAutocorr without the window axis."""
    n, Cn = cells.shape
    L = int(lags)
    if L < 0 or L > _lib.ACF_MAXLAG or L > n - 1:
        raise ValueError("lags = %d outside 0..min(%d, draws - 1 = %d)" % (L, _lib.ACF_MAXLAG, n - 1))
    out = {"acov": np.empty((Cn, L + 1)), "pairs": np.zeros(Cn, dtype=np.int64), "truncated": np.zeros(Cn, dtype=bool)}
    out.update({k: np.empty(Cn) for k in ("mean", "variance", "tau", "ess", "mcse", "rhat")})
    h = n // 2
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for c in range(Cn):
            v = cells[:, c]
            a = v - v[0]
            S1, S2, nn = a.sum(), (a * a).sum(), float(n)
            m = S1 / nn
            out["mean"][c] = v[0] + m
            out["variance"][c] = (S2 - S1 * S1 / nn) / (nn - 1.0)
            H = np.concatenate([[0.0], np.cumsum(a[:L])])
            T = np.concatenate([[0.0], np.cumsum(a[::-1][:L])])
            Cl = np.array([np.dot(a[l:], a[:n - l]) for l in range(L + 1)])
            out["acov"][c] = (Cl - m * (2.0 * S1 - H - T) + (n - np.arange(L + 1)) * m * m) / nn
            out["tau"][c], out["ess"][c], out["mcse"][c], out["pairs"][c], out["truncated"][c] = _geyer(out["acov"][c], out["variance"][c], n)
            f, g, hh = a[:h], a[n - h:], float(h)
            m1, m2 = f.sum() / hh, g.sum() / hh
            v1 = ((f * f).sum() - f.sum() ** 2 / hh) / (hh - 1.0)
            v2 = ((g * g).sum() - g.sum() ** 2 / hh) / (hh - 1.0)
            Wv = (v1 + v2) / 2.0
            mid = a[h:n - h].sum()                   # the draw between the halves of an odd n: 0 unless it is not finite
            out["rhat"][c] = np.sqrt(((((hh - 1.0) / hh) * Wv + (m1 - m2) ** 2 / 2.0) + (mid - mid)) / Wv)
    return out


def calcess(datadir, dates, var="mu", lags=255, result=None):
    """Convergence diagnostics of one variable's chain per end date and column (no reference script computes them): the biased
    autocovariances at lags 0..lags, the integrated autocorrelation time tau by Geyer's initial monotone sequence, the effective
    sample size draws / tau, the Monte-Carlo standard error of the mean and the split-R-hat of the chain's two halves.
    var: mu, sig2, pi_end, A or fcast.

    result=None: every date's per-draw file (`filtered_means_<date>.csv` for mu; see calcchain) is read back and evaluated on
    the host in numpy; no GPU is touched.
    result = a BatchResult of estimatewindows(..., acf_vars=(var, ...), acf_lags=lags): the sums were taken on the device from
    the rounded draws; every date must be one of the result's end dates, and lags must be the result's.
    Returns (dates, ChainAutocorr)."""
    dates = [str(d) for d in dates]
    if var not in DENSITY_FILES:
        raise ValueError("var must be one of %s" % (tuple(DENSITY_FILES),))
    if result is not None:
        d = getattr(result, "autocorr", None)
        if d is None or var not in d:
            raise ValueError("result carries no autocorrelation of %s (estimatewindows(..., acf_vars=(%r,)))" % (var, var))
        d = d[var]
        if int(lags) != d.lags:
            raise ValueError("result was computed for other lags")
        return dates, d.rows(_rows_of(result, dates))
    parts, columns = [], None
    for date in dates:
        columns, cells = _cells(datadir, DENSITY_FILES[var], date)
        parts.append(_autocorr_from_cells(cells, lags))
    return dates, ChainAutocorr(var, columns, {k: np.array([q[k] for q in parts]) for k in ("acov",) + _lib.ACF_FIELDS})


def write_chain_ess(path, dates, diag):
    """`date,column,mean,variance,tau,ess,mcse,pairs,truncated,rhat`: one row per end date and column of a ChainAutocorr.  Our
    layout: the reference writes no such file."""
    rows = []
    for w, d in enumerate(dates):
        for c, name in enumerate(diag.columns):
            rows.append([str(d), name] + [_fmt(getattr(diag, k)[w, c]) for k in ("mean", "variance", "tau", "ess", "mcse")] +
                        [str(int(diag.pairs[w, c])), str(int(diag.truncated[w, c])), _fmt(diag.rhat[w, c])])
    _write_csv(path, ["date", "column", "mean", "variance", "tau", "ess", "mcse", "pairs", "truncated", "rhat"], rows)
    return path


# ------------------------------------------------------------- exact quantiles, credible limits --

def _quantiles_from_cells(cells, probs):
    """The outputs of hmcg_chain_quantiles for one date from the cells (n, C) of its per-draw file, in numpy with the library's
    rule (include/hmcg_order.h): NaNs left out, the rest sorted in the IEEE total order (-0.0 below +0.0: np.sort on the
    order-preserving integer key), h = p (m - 1), j = floor(h), g = h - j, value = lo + g (hi - lo) clamped to hi, one rounded
    operation per step.  Returns the parts of a ChainQuantiles without the window axis."""
    n, Cn = cells.shape
    Q = len(probs)
    out = {k: np.full((Cn, Q), np.nan) for k in _lib.ORD_FIELDS}
    out["count"], out["nan"] = np.zeros(Cn, dtype=np.int64), np.zeros(Cn, dtype=np.int64)
    top = np.uint64(1) << np.uint64(63)
    for c in range(Cn):
        v = np.ascontiguousarray(cells[:, c], dtype=np.float64)
        v = v[~np.isnan(v)]
        m = v.size
        out["count"][c], out["nan"][c] = m, n - m
        if m == 0:
            continue
        u = v.view(np.uint64)
        key = np.sort(np.where(u >> np.uint64(63) != 0, ~u, u | top))
        s = np.where(key >> np.uint64(63) != 0, key & ~top, ~key).view(np.float64)
        for i, p in enumerate(probs):
            h = np.float64(p) * np.float64(m - 1)
            j = int(np.floor(h))
            g = h - np.float64(j)
            lo, hi = s[j], s[min(j + 1, m - 1)]
            with np.errstate(invalid="ignore", over="ignore"):
                if g == 0.0 or lo == hi:
                    value = lo
                else:
                    value = lo + g * (hi - lo)
                    value = hi if value > hi else value
            out["value"][c, i], out["lo"][c, i], out["hi"][c, i], out["g"][c, i] = value, lo, hi, g
    return out


def calcquantiles(datadir, dates, var="mu", probs=(0.05, 0.5, 0.95), result=None):
    """Exact quantiles of one variable's chain per end date and column -- the median and the credible limits a report of the
    fit starts with (numpy's / Julia's default quantile definition).  var: mu, sig2, pi_end, A or fcast.

    result=None: every date's per-draw file (`filtered_means_<date>.csv` for mu; see calcchain) is read back, sorted and
    evaluated on the host in numpy; no GPU is touched.
    result = a BatchResult of estimatewindows(..., quantile_vars=(var, ...), quantile_probs=probs): the values were selected on
    the device from the rounded draws; every date must be one of the result's end dates, and probs must be the result's.
    Returns (dates, ChainQuantiles)."""
    dates = [str(d) for d in dates]
    probs = tuple(float(p) for p in probs)
    if var not in DENSITY_FILES:
        raise ValueError("var must be one of %s" % (tuple(DENSITY_FILES),))
    if not 1 <= len(probs) <= _lib.ORD_MAXQ or not all(0.0 <= p <= 1.0 for p in probs):
        raise ValueError("probs: 1..%d probabilities in [0, 1]" % _lib.ORD_MAXQ)
    if result is not None:
        d = getattr(result, "quantiles", None)
        if d is None or var not in d:
            raise ValueError("result carries no quantiles of %s (estimatewindows(..., quantile_vars=(%r,)))" % (var, var))
        d = d[var]
        if probs != d.probs:
            raise ValueError("result was computed for other probabilities")
        return dates, d.rows(_rows_of(result, dates))
    parts, columns = [], None
    for date in dates:
        columns, cells = _cells(datadir, DENSITY_FILES[var], date)
        parts.append(_quantiles_from_cells(cells, probs))
    return dates, ChainQuantiles(var, columns, probs, {k: np.array([q[k] for q in parts]) for k in _lib.ORD_FIELDS + ("count", "nan")})


def write_chain_quantiles(path, dates, q):
    """`date,column,prob,value,lo,hi,g,count,nan`: one row per end date, column and probability of a ChainQuantiles.  Our
    layout: the reference writes no such file."""
    rows = []
    for w, d in enumerate(dates):
        for c, name in enumerate(q.columns):
            for i, p in enumerate(q.probs):
                rows.append([str(d), name, _fmt(p)] + [_fmt(getattr(q, k)[w, c, i]) for k in _lib.ORD_FIELDS] +
                            [str(int(q.count[w, c])), str(int(q.nan[w, c]))])
    _write_csv(path, ["date", "column", "prob"] + list(_lib.ORD_FIELDS) + ["count", "nan"], rows)
    return path


# ------------------------------------------------- ergodic regime law, durations, long-run moments --

def _ergodic_columns(means, vars_, trans):
    """The per-draw columns (C, n), C = 2K + 2, of hmcg_ergodic_moments from the cells of one date's files -- means, vars_
    (n, K), trans (n, K * K) in the file's column order (trans_i_j, i fastest) -- in numpy by the rule of
    include/hmcg_ergodic.h: the stationary law by the GTH elimination on the off-diagonal cells (the diagonal is never read),
    dur = 1 / the off-diagonal row sum, the long-run mean and variance; one rounded operation per step, in the header's order."""
    n, K = means.shape
    A = np.asarray(trans, dtype=np.float64).reshape(n, K, K).transpose(2, 1, 0)             # A[i, j, d], row i the from-state
    P = [[None if i == j else A[i, j].copy() for j in range(K)] for i in range(K)]
    mu, s2 = np.asarray(means, dtype=np.float64).T, np.asarray(vars_, dtype=np.float64).T
    with np.errstate(all="ignore"):
        dur = []
        for i in range(K):
            cells = [P[i][j] for j in range(K) if j != i]
            s = cells[0]
            for c in cells[1:]:
                s = s + c
            dur.append(1.0 / s)
        for m in range(K - 1, 0, -1):
            S = P[m][0]
            for j in range(1, m):
                S = S + P[m][j]
            for i in range(m):
                P[i][m] = P[i][m] / S
            for i in range(m):
                for j in range(m):
                    if i != j:
                        P[i][j] = P[i][j] + P[i][m] * P[m][j]
        x = [np.ones(n)]
        for j in range(1, K):
            t = x[0] * P[0][j]
            for i in range(1, j):
                t = t + x[i] * P[i][j]
            x.append(t)
        tot = x[0]
        for k in range(1, K):
            tot = tot + x[k]
        pi = [xk / tot for xk in x]
        mean = pi[0] * mu[0]
        for k in range(1, K):
            mean = mean + pi[k] * mu[k]
        within = pi[0] * s2[0]
        for k in range(1, K):
            within = within + pi[k] * s2[k]
        between = None
        for k in range(K):
            e = mu[k] - mean
            t = pi[k] * (e * e)
            between = t if between is None else between + t
        return np.array(pi + dur + [mean, within + between])


def _ergodic_pool(cols):
    """out (C, 2) and n (2,) of hmcg_ergodic_moments from one window's per-draw columns (C, n): mean and variance over the good
    draws (all C values finite) about the pivot, the columns of draw 0 when it is good and zeros otherwise."""
    good = np.isfinite(cols).all(axis=0)
    g = int(good.sum())
    piv = cols[:, 0] if good[0] else np.zeros(cols.shape[0])
    with np.errstate(all="ignore"):
        a = cols[:, good] - piv[:, None]
        S1, S2, gg = a.sum(axis=1), (a * a).sum(axis=1), np.float64(g)
        out = np.stack([piv + S1 / gg, (S2 - S1 * S1 / gg) / (gg - 1.0)], axis=1)
    return out, np.array([g, cols.shape[1] - g], dtype=np.int64)


def calcergodic(datadir, dates, result=None, cols=False):
    """The limit h -> infinity of the regime weights pi_end A^h, per end date: the stationary (ergodic) law of the regimes, the
    expected duration of each regime, and the long-run mean and variance of the series, each as the mean and the variance over
    the draws -- where inflation settles, against which a 12-month forecast is read.  Per draw the law comes from the GTH
    elimination on the off-diagonal cells of the transition matrix (exact to a few roundings on nearly reducible and on
    rounded matrices, where a linear solve is not); a draw with a non-finite column (an absorbing state) is left out and counted.

    result=None: every date's `filtered_means_`, `filtered_variances_` and `filtered_trans_probs_<date>.csv` are read back
    and evaluated on the host in numpy; no GPU is touched.  cols=True adds "cols" (n_dates, 2K + 2, n), the per-draw columns.
    result = a BatchResult of estimatewindows(..., ergodic=True): the values were computed on the device from the rounded
    draws; every date must be one of the result's end dates.
    Returns (dates, e): the dict of _lib.unpack_ergodic over the dates."""
    dates = [str(d) for d in dates]
    if result is not None:
        e = getattr(result, "ergodic", None)
        if e is None:
            raise ValueError("result carries no ergodic moments (estimatewindows(..., ergodic=True))")
        idx = _rows_of(result, dates)
        return dates, {k: v[idx] for k, v in e.items()}
    outs, ns, cls, K = [], [], [], 0
    for date in dates:
        means, vars_, trans = (_cells(datadir, stem, date)[1] for stem in ("filtered_means", "filtered_variances", "filtered_trans_probs"))
        K = means.shape[1]
        c = _ergodic_columns(means, vars_, trans)
        o, n = _ergodic_pool(c)
        outs.append(o), ns.append(n), cls.append(c)
    if not dates:
        return dates, {}
    return dates, _lib.unpack_ergodic(np.array(outs), np.array(ns), K, np.array(cls) if cols else None)


def write_ergodic(path, dates, e):
    """`date,column,mean,variance,good,bad`: one row per end date and per-draw column (pi1.., dur1.., mean, variance) of the
    dict calcergodic returns.  Our layout: the reference writes no such file."""
    K = e["pi_mean"].shape[1]
    names = _lib.erg_names(K)
    rows = []
    for w, d in enumerate(dates):
        mean = list(e["pi_mean"][w]) + list(e["dur_mean"][w]) + [e["mean_mean"][w], e["variance_mean"][w]]
        var = list(e["pi_var"][w]) + list(e["dur_var"][w]) + [e["mean_var"][w], e["variance_var"][w]]
        for c, name in enumerate(names):
            rows.append([str(d), name, _fmt(mean[c]), _fmt(var[c]), str(int(e["good"][w])), str(int(e["bad"][w]))])
    _write_csv(path, ["date", "column", "mean", "variance", "good", "bad"], rows)
    return path


# ------------------------------------------------------- predictive quantiles of the regime mixture: the fan chart --

def _fan_points(lo, hi, M):
    """y_0..y_M of a bracket: step = (hi - lo) / M, y_m = lo + m * step, y_M = hi (include/hmcg_fan.h)."""
    with np.errstate(invalid="ignore", over="ignore"):
        step = (hi - lo) / float(M)
        y = lo + np.arange(M + 1, dtype=np.float64) * step
    y[M] = hi
    return y


def _fan_cell(y, F, p):
    """The cell (lo, hi, Flo, Fhi) below the first point with F >= p, the last cell if there is none (a NaN compares false)."""
    with np.errstate(invalid="ignore"):
        hit = np.flatnonzero(F[1:] >= p)
    m = int(hit[0]) + 1 if hit.size else len(y) - 1
    return y[m - 1], y[m], F[m - 1], F[m]


def _fan_from_cells(means, vars_, pis, trans, probs, horizons, rounds):
    """out (n_h, n_p, 5), range (2,), flag (n_h, n_p) of hmcg_predictive_quantiles from the cells of one date's files -- (n, K)
    each, trans (n, K * K) in the file's column order -- by the rules of include/hmcg_fan.h in float64 numpy: the range
    pass, round 1 on 129 points, rounds of 31 interior points, the cell choice and the finish."""
    n, K = means.shape
    R = _lib.FAN_ROUNDS_DEFAULT if int(rounds) == 0 else int(rounds)
    slab = _lib.PRED_SLAB
    erfc = np.frompyfunc(math.erfc, 1, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        reach = 40.0 * np.sqrt(vars_)
        lo0, hi0 = np.fmin.reduce((means - reach).reshape(-1)), np.fmax.reduce((means + reach).reshape(-1))
        c = 1.0 / (1.4142135623730951 * np.sqrt(vars_))
    out = np.empty((len(horizons), len(probs), _lib.FAN_STRIDE))
    flag = np.zeros((len(horizons), len(probs)), dtype=np.int32)
    for j, h in enumerate(horizons):
        w = _omega(pis, trans, h)

        def F(y):
            with np.errstate(invalid="ignore", over="ignore"):
                f = None
                for k in range(K):
                    ph = 0.5 * erfc(-((y[None, :] - means[:, k, None]) * c[:, k, None])).astype(np.float64)
                    f = w[:, k, None] * ph if k == 0 else w[:, k, None] * ph + f
                tot = np.zeros(len(y))
                for s in range(0, n, slab):                                                 # draw order inside a slab, then slab order
                    tot = tot + np.cumsum(f[s:s + slab], axis=0)[-1]
                return tot / float(n)
        y = _fan_points(lo0, hi0, 128)
        Fy = F(y)
        cells = [_fan_cell(y, Fy, p) for p in probs]
        for _ in range(1, R):
            ys = [_fan_points(b[0], b[1], 32) for b in cells]
            Fi = F(np.concatenate([v[1:32] for v in ys])).reshape(len(probs), 31)
            cells = [_fan_cell(ys[i], np.concatenate(([b[2]], Fi[i], [b[3]])), probs[i]) for i, b in enumerate(cells)]
        for i, ((lo, hi, Flo, Fhi), p) in enumerate(zip(cells, probs)):
            with np.errstate(invalid="ignore", over="ignore"):
                if np.isnan(Flo) or np.isnan(Fhi):
                    q, flag[j, i] = np.nan, _lib.FAN_NAN
                elif not Fhi - Flo > 0.0:
                    q, flag[j, i] = lo, _lib.FAN_FLAT
                elif p > Fhi:
                    q, flag[j, i] = hi, _lib.FAN_UNREACHED
                else:
                    q = lo + (hi - lo) * ((p - Flo) / (Fhi - Flo))
            out[j, i] = (q, lo, hi, Flo, Fhi)
    return out, np.array([lo0, hi0]), flag


def calcfan(datadir, dates, probs, horizons=(0,), result=None, rounds=0):
    """The fan chart: per end date, horizon and probability the quantile of the predictive law -- the mixture of the regimes'
    normals pooled over the draws, whose CDF calccdfs evaluates on a grid -- so the median, the 68 % and 95 % forecast bands
    (probs 0.025, 0.16, 0.5, 0.84, 0.975) and value-at-risk levels come as numbers and not off a plot of `finverse`.
    horizons: 0 = the end date; h > 0 weights the states by pi_i A_i^h.  The CDF is inverted by grid refinement
    (include/hmcg_fan.h): `rounds` rounds, 0 for the default of 4, which leaves |F(q) - p| below 1e-10.

    result=None: every date's `filtered_means_`, `filtered_variances_`, `filtered_state_probs_<date>.csv` (and
    `filtered_trans_probs_<date>.csv` with a horizon > 0) are read back and evaluated on the host in numpy; no GPU is touched.
    result = a BatchResult of estimatewindows(..., fan_probs=probs, fan_horizons=horizons, fan_rounds=rounds): the quantiles
    were computed on the device from the rounded draws; every date must be one of the result's end dates.
    Returns (dates, f): the dict of _lib.unpack_fan over the dates, with probs, horizons and rounds."""
    dates = [str(d) for d in dates]
    probs, horizons = tuple(float(q) for q in probs), tuple(int(h) for h in horizons)
    if result is not None:
        f = getattr(result, "fan", None)
        if f is None:
            raise ValueError("result carries no predictive quantiles (estimatewindows(..., fan_probs=probs))")
        if f["probs"] != probs or f["horizons"] != horizons or f["rounds"] != int(rounds):
            raise ValueError("result was computed for other probabilities, horizons or rounds")
        idx = _rows_of(result, dates)
        return dates, {k: (v[idx] if isinstance(v, np.ndarray) else v) for k, v in f.items()}
    if not 1 <= len(probs) <= _lib.FAN_MAXP or not all(0.0 < q < 1.0 for q in probs):
        raise ValueError("probs: 1..%d probabilities strictly inside (0, 1)" % _lib.FAN_MAXP)
    if not 0 <= int(rounds) <= _lib.FAN_MAXROUNDS:
        raise ValueError("rounds outside 0..%d" % _lib.FAN_MAXROUNDS)
    parts = [_fan_from_cells(*_mixture_cells(datadir, d, horizons), probs, horizons, rounds) for d in dates]
    f = _lib.unpack_fan(np.array([o for o, _, _ in parts]).reshape(len(dates), len(horizons), len(probs), _lib.FAN_STRIDE),
                        np.array([r for _, r, _ in parts]).reshape(len(dates), 2),
                        np.array([g for _, _, g in parts], dtype=np.int32).reshape(len(dates), len(horizons), len(probs)))
    f.update(probs=probs, horizons=horizons, rounds=int(rounds))
    return dates, f


def write_fan(path, dates, f):
    """`date,horizon,p,quantile,lo,hi,flag`: one row per end date, horizon and probability of the dict calcfan returns, float
    text as in the other files (_fmt).  Our layout: the reference writes no such file."""
    rows = [[str(d), str(int(h)), _fmt(p), _fmt(f["quantile"][w, j, i]), _fmt(f["lo"][w, j, i]), _fmt(f["hi"][w, j, i]),
             str(int(f["flag"][w, j, i]))]
            for w, d in enumerate(dates) for j, h in enumerate(f["horizons"]) for i, p in enumerate(f["probs"])]
    _write_csv(path, ["date", "horizon", "p", "quantile", "lo", "hi", "flag"], rows)
    return path


# ------------------------------------------- proper scores of the predictive regime mixture: CRPS, PIT, density --

def _erf(x):
    """erf of a float64 array: scipy's where it is installed, math.erf element by element otherwise."""
    try:
        from scipy.special import erf
    except ImportError:
        return np.frompyfunc(math.erf, 1, 1)(x).astype(np.float64)
    return erf(x)


def _score_a(m, S2):
    """a(m, S2) = E|N(m, S2)| with the steps of include/hmcg_score.h; S2 == 0 gives |m|."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = np.sqrt(S2)
        t = m * (1.0 / (1.4142135623730951 * s))
        a = m * _erf(t) + (s * 0.7978845608028654) * np.exp(-(t * t))
    return np.where(S2 == 0.0, np.abs(m), a)


def _scores_from_cells(means, vars_, pis, trans, horizons, yreal, stride, chunk=1 << 21):
    """out (n_h, 5) of hmcg_predictive_scores from the cells of one date's files -- (n, K) each, trans (n, K * K) in the file's
    column order -- by the formulas of include/hmcg_score.h in float64 numpy over every stride-th draw.  The pair sum runs over
    blocks of rows of the component square of at most `chunk` pairs, so memory stays bounded."""
    n, K = means.shape
    st, n_u = _lib.score_thinning(n, stride)
    means, vars_, pis = means[::st], vars_[::st], pis[::st]
    trans = None if trans is None else trans[::st]
    m, v = means.reshape(-1), vars_.reshape(-1)
    N = m.size
    ws = [_omega(pis, trans, h).reshape(-1) for h in horizons]
    pair = np.zeros(len(horizons))
    rows = max(1, int(chunk) // N)
    for i0 in range(0, N, rows):
        a = _score_a(m[i0:i0 + rows, None] - m[None, :], v[i0:i0 + rows, None] + v[None, :])
        for j, w in enumerate(ws):
            pair[j] += w[i0:i0 + rows] @ (a @ w)
    out = np.empty((len(horizons), _lib.SCORE_STRIDE))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c = 1.0 / (1.4142135623730951 * np.sqrt(v))
        for j, w in enumerate(ws):
            y = float(yreal[j])
            t = (y - m) * c
            e_abs = float(np.sum(w * _score_a(y - m, v))) / n_u
            e_pair = float(pair[j]) / (float(n_u) * float(n_u))
            pit = float(np.sum(w * (0.5 * (1.0 + _erf(t))))) / n_u
            pdf = float(np.sum(w * ((c * 0.5641895835477563) * np.exp(-(t * t))))) / n_u
            out[j] = (e_abs - 0.5 * e_pair, e_abs, e_pair, pit, pdf)
    return out


def calcscores(datadir, dates, horizons, yreal, stride=0, result=None):
    """How good the density forecasts were: per end date and horizon the continuous ranked probability score
    CRPS(F, y) = E|X - y| - 0.5 E|X - X'| of the predictive law F -- the mixture of the regimes' normals pooled over the draws,
    whose CDF calccdfs evaluates -- against the realised value y, with its two parts, the probability integral transform F(y)
    and the predictive density F'(y).  horizons: 0 = the end date; h > 0 weights the states by pi_i A_i^h.  yreal
    (n_dates, n_h): the realised values, NaN for unknown.  stride: every stride-th draw is used (0: thinned to at most 4 096
    draws, 1: every draw); the pair sum costs (draws used * K)^2 / 2 terms per date.

    result=None: every date's `filtered_means_`, `filtered_variances_`, `filtered_state_probs_<date>.csv` (and
    `filtered_trans_probs_<date>.csv` with a horizon > 0) are read back and evaluated on the host in numpy; no GPU is touched.
    result = a BatchResult of estimatewindows(..., score_horizons=horizons, score_stride=stride): the scores were computed on
    the device from the rounded draws against the series' own values (yreal is then not read; the result's is returned); every
    date must be one of the result's end dates.
    Returns (dates, s): the dict of _lib.unpack_scores over the dates, with horizons and stride."""
    dates = [str(d) for d in dates]
    horizons = tuple(int(h) for h in horizons)
    if result is not None:
        sc = getattr(result, "scores", None)
        if sc is None:
            raise ValueError("result carries no scores (estimatewindows(..., score_horizons=horizons))")
        if sc["horizons"] != horizons or sc["stride"] != int(stride):
            raise ValueError("result was computed for other horizons or another stride")
        idx = _rows_of(result, dates)
        return dates, {k: (v[idx] if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
    if not 1 <= len(horizons) <= _lib.HMCG_MAXH or int(stride) < 0:
        raise ValueError("horizons: 1..%d of them; stride >= 0" % _lib.HMCG_MAXH)
    yreal = np.asarray(yreal, dtype=np.float64).reshape(len(dates), len(horizons))
    outs = [_scores_from_cells(*_mixture_cells(datadir, d, horizons), horizons, yreal[w], stride) for w, d in enumerate(dates)]
    sc = _lib.unpack_scores(np.array(outs).reshape(len(dates), len(horizons), _lib.SCORE_STRIDE), yreal.T)
    sc.update(horizons=horizons, stride=int(stride))
    return dates, sc


def write_scores(path, dates, sc):
    """`date,horizon,yreal,crps,e_abs,e_pair,pit,pdf`: one row per end date and horizon of the dict calcscores returns, float
    text as in the other files (_fmt).  Our layout: the reference writes no such file."""
    rows = [[str(d), str(int(h)), _fmt(sc["yreal"][w, j])] + [_fmt(sc[name][w, j]) for name in _lib.SCORE_FIELDS]
            for w, d in enumerate(dates) for j, h in enumerate(sc["horizons"])]
    _write_csv(path, ["date", "horizon", "yreal"] + list(_lib.SCORE_FIELDS), rows)
    return path


def scoresummary(sc, bins=10):
    """Per horizon over the windows with a known realised value (a finite crps): mean_crps (n_h,), count (n_h,) int64 and
    pit_hist (n_h, bins) int64, the PIT histogram on equal bins of [0, 1] (a PIT of 1 counts in the last), flat for a
    calibrated forecast."""
    crps, pit = np.asarray(sc["crps"], dtype=np.float64), np.asarray(sc["pit"], dtype=np.float64)
    known = np.isfinite(crps)
    count = known.sum(axis=0).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(known, crps, 0.0).sum(axis=0) / count
    hist = np.array([np.histogram(pit[known[:, j], j], bins=int(bins), range=(0.0, 1.0))[0] for j in range(crps.shape[1])], dtype=np.int64)
    return {"mean_crps": mean, "count": count, "pit_hist": hist.reshape(crps.shape[1], int(bins))}
