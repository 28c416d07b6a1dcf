"""Device-resident batched estimation: torch is used only for HBM allocation, streams
and torch.distributed plumbing; the sampling is libhmcgibbs (hmcg_estimate_batch_device).
"""
import ctypes as C

import numpy as np

from . import _lib


def panel_shapes(W, ldY, K, nrun, H):
    """The shapes of a DevicePanel's buffers by name: those of the call table (_lib.BUFFERS) for one chain per window."""
    return _lib.call_shapes(_lib.call_dims(W, ldY, K, nrun, H))


class DevicePanel:
    """A window panel resident in HBM plus its output buffers.

    Y (W, ldY) float64, T (W,), yreal (W, H); outputs in the C-ABI layouts
    (include/hmcg.h): mu/sig2/pi_end (W,K,nrun), A (W,K,K,nrun), fcast (W,2H,nrun),
    summary (W, 3K+K^2+2H), status (W,)."""

    def __init__(self, Y, T, K, nrun, horizons=(12,), yreal=None, device=0, window_ids=None, keep_draws=True, corr=False):
        import torch
        if not torch.cuda.is_available():
            raise _lib.HmcgError("no GPU visible to torch: hmc.jl_amd has no CPU fallback")
        _lib.load()
        self.torch = torch
        self.dev = torch.device("cuda", device)
        self.device_index = device
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        self.W, self.ldY = Y.shape
        self.K, self.nrun, self.horizons = int(K), int(nrun), tuple(horizons)
        H = len(self.horizons)
        shape = panel_shapes(self.W, self.ldY, K, nrun, H)
        self.NS = shape["summary"][1]
        self.max_T = int(np.max(T))
        Tv = np.asarray(T)[np.asarray(T) >= 2]
        self.min_T = int(Tv.min()) if Tv.size else 0      # hint for the length-bucketed dispatch (hmcg_config.min_T)
        f64 = dict(dtype=torch.float64, device=self.dev)
        self.Y = torch.from_numpy(Y).to(self.dev)
        self.T = torch.from_numpy(np.ascontiguousarray(T, dtype=np.int32)).to(self.dev)
        self.yreal = None if yreal is None else torch.from_numpy(
            np.ascontiguousarray(yreal, dtype=np.float64).reshape(self.W, H)).to(self.dev)
        self.window_ids = None if window_ids is None else torch.from_numpy(
            np.ascontiguousarray(window_ids, dtype=np.int64).astype(np.int32)).to(self.dev)
        for name in _lib.DRAW_KEYS:
            setattr(self, name, torch.zeros(shape[name], **f64) if keep_draws else None)
        self.summary = torch.zeros(shape["summary"], **f64)
        self.status = torch.zeros(shape["status"], dtype=torch.int32, device=self.dev)
        # extras.corr: correlations between the per-draw outputs (calccorr), needs the draws on the device
        self.corr = torch.zeros(shape["corr"], **f64) if corr else None
        self.last_timing = None
        self._stream = None                # the stream of the latest run (None: the library's own)
        self._held = []                    # input tensors of enqueued library calls: kept until sync() (or a timed call) has waited
        torch.cuda.synchronize(self.dev)   # fills above ran on torch's stream; the library uses its own

    @staticmethod
    def _ptr(t):
        return 0 if t is None else t.data_ptr()

    def run(self, burnin, seed=1234, window_base=0, threads_per_window=0, timed=True, stream=None, bucketed=True):
        """One batched estimate call (burnin + nrun sweeps per window).  With timed=True
        the call waits for completion and returns the HIP-event kernel time in ms.
        bucketed=False withholds the min_T hint: one launch sized for the longest window.
        stream: a raw HIP stream (e.g. torch.cuda.Stream().cuda_stream) to enqueue on; None: the library's own.  The panel
        remembers it: the statistic methods enqueue behind this run, on the same stream."""
        self._stream = stream
        cfg = _lib.make_config(self.W, self.K, self.ldY, self.max_T, burnin, self.nrun, self.horizons, seed,
                               window_base, self.device_index, 0, threads_per_window,
                               min_T=self.min_T if bucketed else 0)
        ex = None
        if self.window_ids is not None or self.corr is not None:
            ex = _lib.Extras()
            ex.struct_size = C.sizeof(_lib.Extras)
            if self.window_ids is not None:
                ex.window_ids = self.window_ids.data_ptr()
            if self.corr is not None:
                ex.corr = self.corr.data_ptr()
        tm = _lib.estimate_batch_device(cfg, self.Y.data_ptr(), self.T.data_ptr(), self._ptr(self.yreal),
                                        self._ptr(self.mu), self._ptr(self.sig2), self._ptr(self.A),
                                        self._ptr(self.pi_end), self._ptr(self.fcast), self.summary.data_ptr(),
                                        self.status.data_ptr(), ex, stream, timed)
        self.last_timing = tm
        return tm.kernel_ms if tm is not None else None

    def _draws(self, what, var="mu", x=None):
        """The panel's HBM draws of `var` for the statistic `what`, and their columns per window.  x: a (W, C, nrun) float64
        tensor on the panel's device to take in their place, e.g. the per-draw columns of ergodic(cols=True)."""
        if x is not None:
            if x.dtype != self.torch.float64 or x.device != self.dev or x.dim() != 3 or x.shape[0] != self.W or x.shape[2] != self.nrun \
                    or not x.is_contiguous():
                raise ValueError("x must be a contiguous float64 (W, C, nrun) tensor on the panel's device")
            self._held.append(x)                # kept until sync(): the enqueued kernels may still read it
            return x, int(x.shape[1])
        if var not in _lib.DRAW_KEYS:
            raise ValueError("var must be one of %s" % (_lib.DRAW_KEYS,))
        x = getattr(self, var)
        if x is None:
            raise _lib.HmcgError("%s needs the draws in HBM: the panel was built with keep_draws=False" % what)
        return x, int(x.numel() // (self.W * self.nrun))

    def _on(self, stream):
        """The stream a statistic is enqueued on: the one given, else that of the latest `run` -- whose draws it reads, so on
        any other stream the caller has to order it behind the run."""
        return self._stream if stream is None else stream

    def _done(self, tm, timed, out):
        """The tail of a statistic: a timed call has waited and leaves its record in last_timing."""
        if timed:
            self.last_timing = tm
        return out

    def predictive_cdf(self, grid, horizons=(0,), timed=False, round5=True, stream=None):
        """Predictive CDFs of the regime mixture from the panel's own HBM draws (hmcg_predictive_cdf_device; calc_cdfs.jl at
        horizon 0, the weights pi_end A^h beyond it): a (W, n_h, G) tensor, the mean over the kept draws per window, horizon
        and grid point.  Enqueued behind `run` on its stream (`stream`: another); with timed=True the call waits and last_timing holds
        the HIP-event time, otherwise call sync() before reading the tensor."""
        self._draws("predictive_cdf")
        torch = self.torch
        g = torch.from_numpy(np.ascontiguousarray(grid, dtype=np.float64).reshape(-1)).to(self.dev)    # a blocking copy
        cdf = torch.empty((self.W, len(horizons), g.numel()), dtype=torch.float64, device=self.dev)
        pred = _lib.make_predictive(self.W, self.K, self.nrun, self.nrun, g.numel(), horizons, self.device_index, round5)
        need_A = any(int(h) > 0 for h in horizons)
        tm = _lib.predictive_cdf_device(pred, self.mu.data_ptr(), self.sig2.data_ptr(), self.pi_end.data_ptr(),
                                        self.A.data_ptr() if need_A else 0, g.data_ptr(), cdf.data_ptr(), self._on(stream), timed)
        self._pred_grid = g                 # kept until the enqueued kernel has read it
        return self._done(tm, timed, cdf)

    def bias_moments(self, horizon=12, timed=False, round5=True, stream=None):
        """Uncertainty-bias moments from the panel's own HBM draws (hmcg_bias_moments_device; bias_calcs.jl:40-53): a
        (W, 2 + 2K + 4K^2) tensor, per window uncbias, totalbias (NaN for a panel without horizons), the mean and the covariance
        of [pi_end A^horizon | mu] over the kept draws (_lib.unpack_bias names the parts of its numpy copy).  Enqueued behind `run`
        on its stream (`stream`: another); with timed=True the call waits and last_timing holds the HIP-event time, otherwise call
        sync() before reading the tensor."""
        self._draws("bias_moments")
        H = len(self.horizons)
        out = self.torch.empty((self.W, _lib.bias_stride(self.K)), dtype=self.torch.float64, device=self.dev)
        bias = _lib.make_bias(self.W, self.K, self.nrun, self.nrun, horizon, H, self.device_index, round5)
        tm = _lib.bias_moments_device(bias, self.mu.data_ptr(), self.pi_end.data_ptr(), self.A.data_ptr() if int(horizon) > 0 else 0,
                                      self.fcast.data_ptr() if H > 0 else 0, out.data_ptr(), self._on(stream), timed)
        return self._done(tm, timed, out)

    def mixture_moments(self, horizons=(0,), timed=False, round5=True, stream=None):
        """Moments of the predictive regime mixture from the panel's own HBM draws (hmcg_mixture_moments_device; skewness.jl
        and alt_forecasts.jl asked of the draws): a (W, n_h, 8) tensor, per window and horizon mean, variance, skewness and
        excess kurtosis of sum_k omega_k N(mu_k, sig2_k), omega = pi_end A^h, pooled over the kept draws, then the mean
        within-draw variance, the variance of the per-draw mean, the mean per-draw skewness and the mean weight
        (_lib.unpack_mixture_moments names the parts of its numpy copy).  Enqueued behind `run` on its stream (`stream`: another); with
        timed=True the call waits and last_timing holds the HIP-event time, otherwise call sync() before reading the tensor."""
        self._draws("mixture_moments")
        hz = tuple(int(h) for h in horizons)
        out = self.torch.empty((self.W, len(hz), _lib.MIX_STRIDE), dtype=self.torch.float64, device=self.dev)
        mix = _lib.make_mixmom(self.W, self.K, self.nrun, self.nrun, hz, self.device_index, round5)
        tm = _lib.mixture_moments_device(mix, self.mu.data_ptr(), self.sig2.data_ptr(), self.pi_end.data_ptr(),
                                         self.A.data_ptr() if any(h > 0 for h in hz) else 0, out.data_ptr(), self._on(stream), timed)
        return self._done(tm, timed, out)

    def chain_density(self, var="mu", cuts=None, bins=64, lo_hi=None, trace=(0, 1), timed=False, round5=True, x=None, stream=None):
        """Chain densities and running means of one variable's draws from the panel's own HBM draws
        (hmcg_chain_density_device; plots/mcplots.jl's plotchain and plotchainmean, plots/timeseriesplots.jl's plot_mean /
        plot_var up to the drawing).  var: "mu", "sig2", "pi_end" (C = K columns), "A" (C = K * K, column i + K * j = A[i, j])
        or "fcast" (C = 2H).  cuts: ascending prefix lengths of the chain (None: the whole chain, (nrun,)); bins equal-width
        bins between lo and hi per window and column, lo_hi (W, C, 2) or None for the range of the finite draws;
        trace = (length, stride) of the running mean.  Returns a dict of tensors: range (W, C, 2), counts
        (W, C, n_cuts, bins + 3) int64 -- the bins, then below, above, nan -- stats (W, C, n_cuts, 2) = mean and variance of each
        prefix, trace (W, C, length); _lib.unpack_chain_density names the parts of their numpy copies.  Enqueued behind `run` on
        its stream (`stream`: another); with timed=True the call waits and last_timing holds the HIP-event time, otherwise call sync()
        before reading the tensors."""
        x, Cn = self._draws("chain_density", var, x)
        torch = self.torch
        dens = _lib.make_density(self.W, Cn, self.nrun, self.nrun, cuts, bins, trace, self.device_index, round5)
        f64 = dict(dtype=torch.float64, device=self.dev)
        lh = None
        if lo_hi is not None:
            lh = torch.from_numpy(np.ascontiguousarray(lo_hi, dtype=np.float64).reshape(self.W, Cn, 2)).to(self.dev)     # a blocking copy
        out = {"range": torch.empty((self.W, Cn, 2), **f64),
               "counts": torch.empty((self.W, Cn, dens.n_cuts, max(int(bins), 0) + 3), dtype=torch.int64, device=self.dev),
               "stats": torch.empty((self.W, Cn, dens.n_cuts, 2), **f64),
               "trace": torch.empty((self.W, Cn, max(int(trace[0]), 0)), **f64)}
        tm = _lib.chain_density_device(dens, x.data_ptr(), 0 if lh is None else lh.data_ptr(), out["range"].data_ptr(),
                                       out["counts"].data_ptr(), out["stats"].data_ptr(),
                                       out["trace"].data_ptr() if dens.trace_len > 0 else 0, self._on(stream), timed)
        if lh is not None and not timed:    # a timed call has waited; otherwise the enqueued kernels may still read it
            self._held.append(lh)
        return self._done(tm, timed, out)

    def chain_autocorr(self, var="mu", lags=255, timed=False, round5=True, x=None, stream=None):
        """Autocovariances and convergence diagnostics of one variable's draws from the panel's own HBM draws
        (hmcg_chain_autocorr_device).  var: "mu", "sig2", "pi_end" (C = K columns), "A" (C = K * K) or "fcast" (C = 2H); lags: the
        largest lag L (0..1024, below nrun).  Returns a dict of tensors: acov (W, C, lags + 1), diag (W, C, 8) = mean, variance,
        tau, ess, mcse, pairs, truncated, rhat; _lib.unpack_chain_autocorr names the parts of their numpy copies.  Enqueued behind `run`
        on its stream (`stream`: another); with timed=True the call waits and last_timing holds the HIP-event time, otherwise call
        sync() before reading the tensors."""
        x, Cn = self._draws("chain_autocorr", var, x)
        torch = self.torch
        acf = _lib.make_autocorr(self.W, Cn, self.nrun, self.nrun, lags, self.device_index, round5)
        f64 = dict(dtype=torch.float64, device=self.dev)
        out = {"acov": torch.empty((self.W, Cn, max(int(lags), 0) + 1), **f64), "diag": torch.empty((self.W, Cn, _lib.ACF_STRIDE), **f64)}
        tm = _lib.chain_autocorr_device(acf, x.data_ptr(), out["acov"].data_ptr(), out["diag"].data_ptr(), self._on(stream), timed)
        return self._done(tm, timed, out)

    def chain_quantiles(self, var="mu", probs=(0.05, 0.5, 0.95), timed=False, round5=True, x=None, stream=None):
        """Exact quantiles of one variable's draws from the panel's own HBM draws (hmcg_chain_quantiles_device): a selection on
        the device, no draw leaves it.  x: a (W, C, nrun) tensor to take in place of a variable (see _draws).  var: "mu", "sig2", "pi_end" (C = K columns), "A" (C = K * K) or "fcast" (C = 2H); probs:
        at most 16 probabilities in [0, 1].  Returns a dict of tensors: q (W, C, Q, 4) = value, lo, hi, g per probability and
        n (W, C, 2) int64 = the draws ranked and the NaNs; _lib.unpack_chain_quantiles names the parts of their numpy copies.
        Enqueued behind `run` on its stream (`stream`: another); with timed=True the call waits and last_timing holds the HIP-event time,
        otherwise call sync() before reading the tensors."""
        x, Cn = self._draws("chain_quantiles", var, x)
        torch = self.torch
        qs = _lib.make_quantiles(self.W, Cn, self.nrun, self.nrun, probs, self.device_index, round5)
        out = {"q": torch.empty((self.W, Cn, qs.Q, _lib.ORD_STRIDE), dtype=torch.float64, device=self.dev),
               "n": torch.empty((self.W, Cn, 2), dtype=torch.int64, device=self.dev)}
        tm = _lib.chain_quantiles_device(qs, x.data_ptr(), out["q"].data_ptr(), out["n"].data_ptr(), self._on(stream), timed)
        return self._done(tm, timed, out)

    def ergodic(self, cols=False, timed=False, round5=True, stream=None):
        """The ergodic regime law, expected durations and long-run mean and variance from the panel's own HBM draws
        (hmcg_ergodic_moments_device): the limit h -> infinity of the weights pi_end A^h.  Returns a dict of tensors: out
        (W, 2K + 2, 2) = mean and variance over the good draws of pi[K], dur[K], the long-run mean and the long-run variance,
        n (W, 2) int64 = the good draws (every column finite) and the rest, and with cols=True cols (W, 2K + 2, nrun), the
        per-draw columns, which chain_quantiles / chain_density / chain_autocorr take as x=; _lib.unpack_ergodic names the
        parts of their numpy copies.  Enqueued behind `run` on its stream (`stream`: another); with timed=True the call waits and
        last_timing holds the HIP-event time, otherwise call sync() before reading the tensors."""
        self._draws("ergodic")
        torch = self.torch
        Cn = _lib.erg_cols(self.K)
        erg = _lib.make_ergodic(self.W, self.K, self.nrun, self.nrun, self.device_index, round5)
        out = {"out": torch.empty((self.W, Cn, 2), dtype=torch.float64, device=self.dev),
               "n": torch.empty((self.W, 2), dtype=torch.int64, device=self.dev)}
        if cols:
            out["cols"] = torch.empty((self.W, Cn, self.nrun), dtype=torch.float64, device=self.dev)
        tm = _lib.ergodic_moments_device(erg, self.mu.data_ptr(), self.sig2.data_ptr(), self.A.data_ptr(),
                                         out["cols"].data_ptr() if cols else 0, out["out"].data_ptr(), out["n"].data_ptr(), self._on(stream), timed)
        return self._done(tm, timed, out)

    def fan(self, probs, horizons=(0,), rounds=0, timed=False, round5=True, stream=None):
        """Quantiles of the predictive regime mixture from the panel's own HBM draws (hmcg_predictive_quantiles_device): per
        window, horizon and probability the quantile of the law whose CDF predictive_cdf evaluates -- the median, the forecast
        bands of a fan chart, value-at-risk levels --, by `rounds` rounds of grid refinement (0: the default, 4).  Returns a
        dict of tensors: out (W, n_h, n_p, 5) = quantile, lo, hi, Flo, Fhi, range (W, 2) and flag (W, n_h, n_p) int32;
        _lib.unpack_fan names the parts of their numpy copies.  Enqueued behind `run` on its stream (`stream`: another); with timed=True
        the call waits and last_timing holds the HIP-event time, otherwise call sync() before reading the tensors."""
        self._draws("fan")
        torch = self.torch
        hz = tuple(int(h) for h in horizons)
        fan = _lib.make_fan(self.W, self.K, self.nrun, self.nrun, probs, hz, rounds, self.device_index, round5)
        out = {"out": torch.empty((self.W, fan.n_h, fan.n_p, _lib.FAN_STRIDE), dtype=torch.float64, device=self.dev),
               "range": torch.empty((self.W, 2), dtype=torch.float64, device=self.dev),
               "flag": torch.empty((self.W, fan.n_h, fan.n_p), dtype=torch.int32, device=self.dev)}
        tm = _lib.predictive_quantiles_device(fan, self.mu.data_ptr(), self.sig2.data_ptr(), self.pi_end.data_ptr(),
                                              self.A.data_ptr() if any(h > 0 for h in hz) else 0, out["out"].data_ptr(),
                                              out["range"].data_ptr(), out["flag"].data_ptr(), self._on(stream), timed)
        return self._done(tm, timed, out)

    def scores(self, horizons, yreal=None, stride=0, timed=False, round5=True, stream=None):
        """Proper scores of the predictive regime mixture from the panel's own HBM draws (hmcg_predictive_scores_device): per
        window and horizon the continuous ranked probability score against yreal, its parts E|X - y| and E|X - X'|, the
        probability integral transform F(y) and the predictive density at y.  yreal: (n_h, W), NaN for unknown (None: all
        unknown, which leaves e_pair, the forecast's Gini mean difference).  stride: every stride-th kept draw is used; 0: the
        default thinning to at most 4 096 draws, 1: the exact score, whose cost grows with the square of nrun * K.  Returns a
        (W, n_h, 5) tensor = crps, e_abs, e_pair, pit, pdf; _lib.unpack_scores names the parts of its numpy copy.  Enqueued behind
        `run` on its stream (`stream`: another); with timed=True the call waits and last_timing holds the HIP-event time, otherwise
        call sync() before reading the tensor."""
        self._draws("scores")
        torch = self.torch
        hz = tuple(int(h) for h in horizons)
        sc = _lib.make_score(self.W, self.K, self.nrun, self.nrun, hz, stride, self.device_index, round5)
        y = torch.from_numpy(_lib._score_yreal(yreal, sc.n_h, self.W)).to(self.dev)             # a blocking copy
        out = torch.empty((self.W, sc.n_h, _lib.SCORE_STRIDE), dtype=torch.float64, device=self.dev)
        tm = _lib.predictive_scores_device(sc, self.mu.data_ptr(), self.sig2.data_ptr(), self.pi_end.data_ptr(),
                                           self.A.data_ptr() if any(h > 0 for h in hz) else 0, y.data_ptr(), out.data_ptr(), self._on(stream), timed)
        if not timed:                       # a timed call has waited; otherwise the enqueued kernels may still read it
            self._held.append(y)
        return self._done(tm, timed, out)

    def sync(self):
        """Wait for everything enqueued on the device, whichever stream it went to (untimed calls are asynchronous)."""
        self.torch.cuda.synchronize(self.dev)
        del self._held[:]
