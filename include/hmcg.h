/*
 * hmcg.h -- C ABI of libhmcgibbs.so: batched Gibbs-sampled Gaussian-HMM estimation
 * on AMD MI355X (gfx950).  This is the drop-in boundary for the data-parallel hot
 * path of joe5saia/Hmc.jl.
 *
 * The reference has no FFI of its own: its boundary is the Julia function surface
 * of `module Hmc`.  What each entry point replaces (reference file:line):
 *
 *   hmcg_estimate_batch[_device]   W x { Hmc.estimatemodel(opt)       src/Hmc.jl:850-865
 *                                        -> makeParams                src/Hmc.jl:161-195
 *                                        -> HyperParams(Y,D)          src/Hmc.jl:132-142
 *                                        -> gibbssample!/gibbssweep!  src/Hmc.jl:486-562
 *                                           (update_mu_sigma :231-336, update_beta :338-348,
 *                                            update_rho :350-356, update_A :358-369,
 *                                            forwardupdate_P :371-440, backwardupdate_P :442-457
 *                                            [only pib[end,:] is produced], sort :501-513,
 *                                            update_X :459-484)
 *                                        -> forecast per draw         src/Hmc.jl:658-667, 860-862 }
 *                                  and the per-window means that runaggregate
 *                                  (src/Hmc.jl:1025-1078) takes over the 5-digit-rounded
 *                                  per-draw CSV rows of basicsave (src/Hmc.jl:707-722).
 *   W windows in one call          replace the SLURM array fan-out, one process per
 *                                  window (slurmscripts/base_estimation.sh:5,17).
 *   hmcg_predictive_cdf[_device]   code/hassan_cdfs/calc_cdfs.jl:31-42: per end date the mean over the draws of the
 *                                  regime mixture's normal CDF on a grid of points (`expectationsbar`), taken from the
 *                                  draw arrays instead of the three per-draw CSV files it reads back; with horizons > 0
 *                                  the same mixture under the h-step state law pi_end * A^h of forecast (src/Hmc.jl:662-663).
 *   hmcg_bias_moments[_device]     code/hassan_cdfs/bias_calcs.jl:40-53 (calcbias): per end date the mean and covariance over
 *                                  the draws of [pi_end * A^12 | mu] and the two numbers it reduces them to (uncerbias,
 *                                  totalbias), taken from the draw arrays instead of the four per-draw CSV files it reads back.
 *   hmcg_mixture_moments[_device]  code/skewness.jl:31-43 and code/alt_forecasts.jl:30-35, asked of the draws instead of the
 *                                  summary rows: mean, variance, skewness and excess kurtosis of the predictive law
 *                                  sum_k omega_k N(mu_k, sig2_k), omega = pi_end * A^h, pooled over the draws in closed form
 *                                  (skewness.jl estimates one third moment from 10 000 000 variates of the plug-in mixture;
 *                                  alt_forecasts.jl sets the plug-in mean beside the draw mean), and what a plug-in hides:
 *                                  the within- and between-draw shares of the variance and the mean per-draw skewness.
 *   hmcg_chain_density[_device]    plots/mcplots.jl:24-38 (plotchain: the density of one parameter's draws over the nested
 *                                  prefixes 1:100_000 .. 1:250_000 of the chain), :47-63 (plotchainmean: the cumulative mean of
 *                                  a column over the first 10 000 draws) and plots/timeseriesplots.jl:83-142 (plot_mean /
 *                                  plot_var: the marginal posterior densities of the state means and variances) up to the
 *                                  drawing: per window and draw column the binned counts of every prefix, its mean and
 *                                  variance, and the running mean, taken from the draw arrays instead of the per-draw CSV
 *                                  files the scripts read back.
 *   hmcg_chain_autocorr[_device]   no reference script: the convergence diagnostics a user of the sampler asks for next --
 *                                  per window and draw column the autocovariances up to a largest lag, the integrated
 *                                  autocorrelation time by Geyer's initial monotone sequence, the effective sample size, the
 *                                  Monte-Carlo standard error of the mean and the split-R-hat of the chain's two halves.
 *
 * Conventions: plain C structs, fixed-width ints, no C++ types or exceptions cross
 * the boundary.  Return 0 on success, negative on API misuse (HMCG_E_*), positive
 * = hipError_t of a failed HIP call.  Per-window numerical trouble is reported in
 * status[w] (HMCG_ST_* bits), never as a call failure.  The caller allocates and
 * owns every buffer; the library keeps no caller pointer after return.  The host
 * entries are blocking.  The library keeps one lazily created context per device (streams, events,
 * grow-only device and pinned-host workspaces; hmcg_shutdown releases them); calls on the SAME device are
 * serialised by that context's mutex, calls on different devices run concurrently.  There is NO CPU
 * fallback: without a usable GPU every compute entry fails with HMCG_E_NODEVICE.
 *
 * Array layouts are the reference's Julia (column-major) layouts with the window
 * index appended as the slowest dimension:
 *   mu, sig2, pi_end : Julia (nrun, K, W)      elem (d,k,w)   at d + nrun*(k + K*w)
 *   A                : Julia (nrun, K, K, W)   elem (d,i,j,w) at d + nrun*(i + K*(j + K*w))
 *   fcast            : Julia (nrun, 2H, W)     cols forecast_h, forecast_error_h per horizon
 *   summary          : Julia (3K+K*K+2H, W)    means over draws of round(x; digits=5), rows
 *                      mu(K) | sig2(K) | pi_end(K) | A(:) column-major (K*K) | fcast(2H)
 *   Y                : window-major panel, row w holds Y_w[0..T[w]-1], leading dim ldY
 *   yreal            : (H, W): realised value rawdata[endIndex+h] per horizon (NaN if unknown)
 * "sig2" holds the VARIANCE draws (the reference's `sigma` arrays hold variances).
 * States are labelled 0..K-1 here (1..K in Julia).
 */
#ifndef HMCG_H
#define HMCG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HMCG_VERSION 109
#define HMCG_MAXH 8
#define HMCG_MAXTAIL 256        /* most signal steps past the end date (sigLen, src/Hmc.jl:888) */
#define HMCG_MAXK 8
#define HMCG_MAXDEV 16           /* devices one process may drive */

/* API-misuse return codes */
#define HMCG_E_BADARG   (-1)
#define HMCG_E_NODEVICE (-2)
#define HMCG_E_UNSUPPORTED (-3) /* (K, max_T) combination has no compiled kernel */
#define HMCG_E_NOMEM    (-4)

/* status[w] bits */
#define HMCG_ST_BAD_INVGAMMA   1 /* a<=0 or b<=0 in the InvGamma update: old variance kept (src/Hmc.jl:319-329).  Kept for the
                                    reference's branch; no call can raise it: the entry reads alpha <= 0 as 1, so a >= alpha > 0,
                                    and beta >= 1 plus non-negative sums of squares keeps b > 0.  No test provokes it. */
#define HMCG_ST_EMIS_UNDERFLOW 2 /* all K emission pdfs underflowed at some step: that observation was treated as missing (f=1); or a zero
                                    normaliser was replaced by the uniform law (reference would produce NaN and throw, src/Hmc.jl:435) */
#define HMCG_ST_NONFINITE      4 /* non-finite observation: window skipped, outputs untouched */
#define HMCG_ST_GAMMA_CAP      8 /* gamma rejection sampler hit its attempt cap */
#define HMCG_ST_BAD_T         16 /* T[w] < 2, T[w] > ldY, T[w] beyond what max_T was sized for, or end_pos[w] outside
                                      [T-1-HMCG_MAXTAIL, T-1]: window skipped */
#define HMCG_ST_BAD_RANGE     32 /* signal path: sig_range[w] / save_range[w] outside [0, T[w]], a non-empty sig_range not ending
                                      at T[w], or a save_range longer than nsave_ld: window skipped */

/* flags */
#define HMCG_FLAG_RESUME 1  /* chain state (extras.xstate) is loaded instead of the makeParams init; sweep numbering continues at sweep_base */

typedef struct hmcg_config {
    int32_t struct_size;     /* = sizeof(hmcg_config), for ABI evolution */
    int32_t W;               /* windows in this call */
    int32_t K;               /* states, 2..HMCG_MAXK   (estopt.D, src/Hmc.jl:32) */
    int32_t ldY;             /* leading dimension of the Y panel, >= max_T */
    int32_t max_T;           /* max over w of T[w] (0: use ldY) */
    int32_t burnin;          /* discarded sweeps (estopt.burnin, src/Hmc.jl:33) */
    int32_t nrun;            /* kept sweeps      (estopt.Nrun,   src/Hmc.jl:34) */
    int32_t H;               /* number of forecast horizons, 0..HMCG_MAXH */
    int32_t horizons[HMCG_MAXH]; /* estopt.horizons, src/Hmc.jl:31 */
    uint64_t seed;           /* estopt.seed (src/Hmc.jl:41,59); Philox key */
    uint32_t window_base;    /* RNG stream id of window 0 of this call; window w uses window_base+w,
                                so a sharded run reproduces the unsharded one */
    int32_t device;          /* HIP device ordinal */
    int32_t flags;           /* HMCG_FLAG_* */
    int32_t threads_per_window; /* 0 = auto (256); 128/256/512 */
    int32_t sweep_base;      /* global index of the first sweep of this call (0 unless resuming) */
    int32_t sweep_count;     /* sweeps to run in this call; 0 = all remaining (burnin+nrun-sweep_base).  A call that
                                stops short writes extras.xstate/sumacc so a later RESUME call can continue */
    double alpha;            /* InvGamma prior sample size, 0 -> 1.0 (HyperParams(Y,D), src/Hmc.jl:137; 2.0 for HyperParams(opt) :154) */
    double nu;               /* Normal prior sample size,   0 -> 1.0 (src/Hmc.jl:140; 2.0 for HyperParams(opt) :157) */
    /* signal Monte-Carlo path (estimatesignals!, src/Hmc.jl:868-914); leave zero for estimatemodel */
    double kappa;            /* hp.kappa: relative noise of a signal observation (opt.noise :158; 1.0 in the base run :132) */
    int32_t n_samples;       /* opt.noiseSamples: consecutive chains of burnin+nrun sweeps, each on fresh noise, the chain
                                state carried over (:889-895); 0 or 1 = a single chain.  Outputs then hold n_samples*nrun
                                draws (sample-major), burnin/nrun being opt.signalburnin/opt.signalNrun */
    int32_t blend_mask;      /* signal path: bit k set = horizon k equals sigLen and is reported through forecastsignal
                                (src/Hmc.jl:670-681, :908-909): sum_i pi_last[i] (a Yfake[T-1] + (1-a) mu[i]), a = tau/(1+tau),
                                tau = 1/sigma_signal[w]; horizons[k] is then ignored.  0 otherwise */
    int32_t min_T;           /* device entry, optional hint: min over w of T[w] (0: unknown).  With it a ragged batch -- the
                                reference's production run is 460 expanding windows of 120..579 months, code/run_hmm.jl:79-109 --
                                is dispatched by length: every window runs on the steps-per-thread variant its OWN length
                                selects (one launch per length class, side by side), and its result is that of a call with
                                this window alone.  Without it one launch is sized for max_T.  The host entries read T
                                themselves and ignore the field */
    int32_t reserved3;
} hmcg_config;

/* Optional debug / teacher-forcing / checkpoint buffers (all may be NULL).  Pointer
 * residency follows the entry point (host pointers for hmcg_estimate_batch, device
 * pointers for hmcg_estimate_batch_device). */
typedef struct hmcg_extras {
    int32_t struct_size;
    int32_t reserved;
    const int32_t* x_init;   /* [W][ldY] initial states (0-based) instead of makeParams' argmax-pdf init */
    int32_t* x_final;        /* [W][ldY] states after the last sweep */
    double* pif_final;       /* [W][ldY][K] UNSORTED filtered probabilities pif[t,:] of the last sweep */
    uint8_t* xstate;         /* [W][ldY] chain state for HMCG_FLAG_RESUME: read at start when the flag is
                                set, written at the end whenever non-NULL (checkpoint) */
    double* sumacc;          /* [W][3K+K*K+2H+K] checkpoint block: the running sums behind `summary`, then the K pivots of
                                the one-pass sufficient statistics (so that a resumed chain is bit-identical) */
    const uint32_t* window_ids; /* [W] explicit RNG stream ids (NULL: window_base + w); lets a sharded /
                                   load-balanced run reproduce the unsharded one window for window */
    /* signal path (all NULL for estimatemodel).  Positions are 0-based and window-relative. */
    const int32_t* sig_range;   /* [W][2] signal positions [begin, end): opt.signalRange; end must equal T[w] */
    const int32_t* save_range;  /* [W][2] positions reported in sigvals: opt.signalSave */
    const double* sigma_signal; /* [W] opt.sigma_signal: sd of the N(0,1) noise added to the signal positions (:892) */
    double* sigvals;            /* [W][n_samples][nsave_ld] Yfake[signalSave] of every noise sample (:904) */
    int32_t nsave_ld;
    int32_t reserved2;
    const int32_t* end_pos;     /* [W] signal path, optional: position (opt.endIndex - 1) whose SMOOTHED probabilities are
                                   reported in pi_end when the window carries sigLen = T-1-end_pos signal steps past the end
                                   date (samples.pib[:, opt.endIndex, :], src/Hmc.jl:888,900); 0 <= sigLen <= HMCG_MAXTAIL.
                                   NULL: the last step.  Forecasts always start from the last step (:907,909): pass
                                   horizons[k] = h - sigLen, or set blend_mask for h == sigLen */
    double* pi_smooth_mean;     /* [W][ldY][K] optional: mean over the kept draws of the SMOOTHED probabilities
                                   P(X_t | Y_1:T, theta) in sorted labels = the draw-average of the reference's
                                   samples.pib[:, t, :] (backwardupdate_P!, src/Hmc.jl:442-457, sorted :513).  Every K and every
                                   supported T (the LDS-resident kernel needs extras.pif_final on the device entry); about
                                   half as many draws per second as without.  NULL: only pib[end,:] is produced.
                                   Buffer contents: a call without HMCG_FLAG_RESUME does not depend on what pi_smooth_mean /
                                   pi_filter_mean hold on entry (the chain's running sums start at zero on every kernel; steps
                                   t >= T[w] and skipped windows are left untouched).  A call that stops short (sweep_count)
                                   leaves the raw running sums in them; the RESUME call that continues it reads them back
                                   from the same buffers and the call that ends the run turns them into means */
    double* pi_filter_mean;     /* [W][ldY][K] optional: the same draw average for the FILTERED probabilities pif[t,:] in
                                   sorted labels (what the reference's older API returned as "pib" and averaged per date in
                                   data/output/official_insample/forecats_insample.csv, columns s1..s3).  Runs on the same
                                   kernel variants as pi_smooth_mean */
    double* corr;               /* [W][NC][NC] optional, NC = HMCG_CORR_COLUMNS(K): Pearson correlations between the per-draw
                                   outputs of each window over its kept draws, columns mu_1..K | sigma_1..K | pi_1..K |
                                   vec(A) column-major | forecast of horizons[0] -- the matrix calccorr (src/Hmc.jl:1094-1163)
                                   computes per end date from the 5-digit-rounded per-draw CSV files, here taken from the
                                   rounded draws while they are in HBM (second moments about the first draw, accumulated in
                                   draw order, chunk by chunk).  Needs all five per-draw outputs (mu, sig2, A, pi_end, fcast
                                   with H >= 1; the host entries accept NULL for them and then keep the draws on the device),
                                   n_samples <= 1 and the whole run in one call (no sweep_base / sweep_count / RESUME).  A
                                   constant column gives NaN, as Statistics.cor does */
    double* pi_smooth_draws;    /* [W][K][ldY][nd] = Julia (Nrun, N, D, W), optional: EVERY kept draw's smoothed probabilities in sorted
                                   labels -- the reference's samples.pib[Nrun, N, D] itself (gibbssample!, src/Hmc.jl:552,558), of
                                   which its live outputs only read [:, end, :] (= pi_end).  8 K T bytes per draw and window (24 KB at
                                   K = 3, T = 1000): the host entries stream it chunk by chunk like the other per-draw outputs.  Runs the
                                   smoothing variants, as pi_smooth_mean does */
    double* sample_summary;     /* [W][n_samples][3K+K*K+2H] optional, signal path: for every noise sample the mean over its
                                   nrun kept draws of the 5-digit-rounded outputs, columns as in `summary` -- one row of the
                                   `*_summary.csv` files upstream's runaggregate (src/Hmc.jl:1025-1057, grouped by date and
                                   signalid) makes out of a signal run's per-draw files, taken on the device instead (the
                                   n_samples * nrun draws need not leave it).  While a sample is incomplete (a call that
                                   stops inside it: sweep_count) its row holds the raw running sums; a RESUME call reads
                                   them back from the same buffer */
} hmcg_extras;
#define HMCG_CORR_COLUMNS(K) (3 * (K) + (K) * (K) + 1)

typedef struct hmcg_timing {
    double kernel_ms;        /* HIP-event time of the sweep kernel(s) on the launch stream (summed over the chunks of a call) */
    int32_t launches;        /* kernel launches of this call: the host entries run a long chain in chunks whose per-draw
                                outputs travel to the caller while the next chunk samples */
    int32_t threads_per_window;
    int32_t steps_per_thread;
    int32_t lds_bytes;
    int32_t helper_waves;    /* extra 64-thread waves per window that carry the draw-phase side jobs (0 or 4) */
    int32_t device;          /* HIP device ordinal this record describes */
    double call_ms;          /* host entries: wall time of the whole call on this device -- staging, H2D, kernels, D2H and the
                                scatter into the caller's arrays (0 for the device entry) */
    int32_t windows;         /* windows this device ran */
    int32_t occupancy;       /* register-resident kernels: 1 = the whole register file per window, 2 = capped so that two windows
                                share a CU (the OCC template argument of the kernel that ran); 0 for the LDS-resident kernel */
    int32_t buckets;         /* length classes the call was dispatched in (1: one launch for every window); threads_per_window,
                                steps_per_thread, helper_waves, occupancy and lds_bytes then describe the LONGEST class */
    int32_t streaming;       /* 1: the LDS-resident kernel ran in its HBM-streaming form (window longer than a CU's LDS holds) */
} hmcg_timing;

int hmcg_version(void);
int hmcg_device_count(void);          /* number of usable HIP devices (0 if none) */
const char* hmcg_last_error(void);    /* thread-local, never NULL */
void hmcg_shutdown(void);             /* releases the library's streams/workspaces */

/* Host-buffer entry: stages Y/T/yreal through pinned memory to the device, runs the chain in a few chunks and
 * streams each chunk's per-draw outputs back (SDMA copy into pinned staging, then into the caller's arrays)
 * while the next chunk samples.  Any output pointer may be NULL (that output is not produced).  Outputs of
 * skipped windows (status HMCG_ST_NONFINITE / HMCG_ST_BAD_T / HMCG_ST_BAD_RANGE) are zero here; the device entry
 * leaves them untouched. */
int hmcg_estimate_batch(const hmcg_config* cfg, const double* Y, const int32_t* T, const double* yreal,
                        double* mu, double* sig2, double* A, double* pi_end, double* fcast,
                        double* summary, int32_t* status, const hmcg_extras* extras, hmcg_timing* timing);

/* Device-buffer entry: every data pointer is HBM-resident on cfg->device.  Work is
 * enqueued on `stream` (a hipStream_t; NULL = the library's own stream).  The call
 * returns after enqueueing unless `timing` is non-NULL, in which case it waits for
 * completion and fills it.  status must be zero-initialised by the caller or is
 * zeroed by the library when HMCG_FLAG_RESUME is not set. */
int hmcg_estimate_batch_device(const hmcg_config* cfg, const double* dY, const int32_t* dT, const double* dyreal,
                               double* dmu, double* dsig2, double* dA, double* dpi_end, double* dfcast,
                               double* dsummary, int32_t* dstatus, const hmcg_extras* dextras,
                               void* stream, hmcg_timing* timing);

/* Multi-device host entry: the same contract as hmcg_estimate_batch, with the W windows of the call partitioned over
 * n_devices GPUs of this node -- what the reference does with one SLURM array task per end date
 * (slurmscripts/base_estimation.sh:5,17: `--array=120-579`, one Julia process per window).  Windows are independent
 * chains, so the data path has no collective: the library sorts the windows by length, deals them to the lightest
 * device (count-balanced), runs one host thread + stream + workspace per device, keys every window's random numbers by
 * its GLOBAL id (extras.window_ids[w], or cfg->window_base + w) -- so the result is bit-identical to the
 * single-device call whatever the partition -- and each device's thread places its windows' blocks straight into the
 * caller's arrays (the gather).  cfg->device is ignored; device_ids lists distinct HIP ordinals (NULL: 0..n_devices-1).
 * timing, if not NULL, receives n_devices records.  Returns 0, an HMCG_E_* code, or the hipError_t of the first
 * device that failed (hmcg_last_error() names it). */
int hmcg_estimate_batch_multi(const hmcg_config* cfg, int32_t n_devices, const int32_t* device_ids,
                              const double* Y, const int32_t* T, const double* yreal,
                              double* mu, double* sig2, double* A, double* pi_end, double* fcast,
                              double* summary, int32_t* status, const hmcg_extras* extras, hmcg_timing* timing);

/* ---- predictive CDFs of the regime mixture (calc_cdfs.jl) ----------------------------------------------------------------
 * cdf[w][j][g] = mean over the nd draws d of  sum_k omega_{d,j}[k] * Phi((grid[g] - mu_d[k]) / sqrt(sig2_d[k])),
 * omega_{d,j} = pi_end_d * A_d^h_j, built by h_j successive row-vector x matrix products (k ascending in every dot product),
 * Phi(z) = erfc(-z / sqrt 2) / 2 as StatsFuns.normcdf computes it.  horizons[j] = 0 is the end date itself: calc_cdfs.jl:39-41,
 * `expectationsbar` of one end date on ys = grid.  The draw arrays are those of the estimate entries (layouts above) with
 * leading dimension nd_ld >= nd: element (d, k, w) at d + nd_ld * (k + K * w), A's (d, i, j, w) at d + nd_ld * (i + K * (j + K * w)).
 * HMCG_PRED_ROUND5: every input (draws and grid) is first rounded as basicsave rounds a CSV cell (round(x; digits=5)), so the
 * values are the cells upstream reads back; without it the raw draws are used.  IEEE cases fall as they do in Julia: a
 * variance of 0 gives Phi = 0 or 1 and NaN where grid[g] == mu; a NaN term makes its cell NaN even under a zero weight.
 * Deterministic: the draws are reduced in fixed slabs of draws, in draw order inside a slab and slab by slab after that (no
 * floating-point atomics), so the result is bit-identical from run to run, from both entries, and however the host entry
 * cuts its upload into chunks (HMCG_CHUNK_DRAWS under HMCG_DIAG=1, rounded up to whole slabs).
 * Misuse (HMCG_E_BADARG, checked before any HIP call): struct_size, K outside 2..HMCG_MAXK, G outside 1..HMCG_MAXGRID, n_h
 * outside 1..HMCG_MAXH, a horizon outside 0..HMCG_PRED_MAXH, W < 1, nd < 1, nd_ld < nd, a NULL mu / sig2 / pi_end / grid /
 * cdf, NULL A with a horizon > 0; the host entry also refuses a non-finite grid point. */
#define HMCG_PRED_ROUND5 1
#define HMCG_MAXGRID 4096
#define HMCG_PRED_MAXH 1024            /* largest horizon */
typedef struct hmcg_predictive {
    int32_t struct_size, W, K, device;
    int64_t nd, nd_ld;                 /* draws per window; leading dimension of the draw arrays (>= nd) */
    int32_t G, n_h;                    /* grid points 1..HMCG_MAXGRID; horizons 1..HMCG_MAXH */
    int32_t horizons[HMCG_MAXH];       /* 0 = the end date itself (calc_cdfs.jl) */
    int32_t flags, reserved;
} hmcg_predictive;
/* Device entry: every data pointer is HBM-resident on p->device; enqueued on `stream` (NULL: the library's own) behind the
 * library's earlier work there; returns after enqueueing unless `timing` is given (kernel_ms: HIP events around the kernels). */
int hmcg_predictive_cdf_device(const hmcg_predictive* p, const double* dmu, const double* dsig2, const double* dpi_end,
                               const double* dA /* NULL iff every horizon is 0 */, const double* dgrid,
                               double* dcdf /* [W][n_h][G] */, void* stream, hmcg_timing* timing);
/* Host entry (blocking): uploads the draws in chunks of whole slabs through pinned staging, the copy of one chunk beside the
 * kernel of the one before. */
int hmcg_predictive_cdf(const hmcg_predictive* p, const double* mu, const double* sig2, const double* pi_end,
                        const double* A, const double* grid, double* cdf, hmcg_timing* timing);

/* ---- uncertainty-bias moments of the draws (bias_calcs.jl) ------------------------------------------------------------------
 * Per window, over its nd draws d (code/hassan_cdfs/bias_calcs.jl:40-53, `calcbias`):
 *   futstate_d = pi_end_d * A_d^horizon   h successive row-vector x matrix products, k ascending in every dot product: the same
 *                                         bits as the weights of hmcg_predictive_cdf (upstream: states[i,:]' * reshape(trans[i,:],3,3)^12)
 *   v_d        = [futstate_d | mu_d]      2K columns
 *   mean       = mean over d of v_d;  cov = cov(v), divisor nd - 1 (`covv = cov(hcat(futstate, means))`)
 *   nab        = [mean of mu | mean of futstate]           (`nab = mean(hcat(means, futstate), dims=1)`: the OTHER column order)
 *   uncbias    = nab * cov * nab'     exactly as upstream writes it: nab is ordered means | futstate while cov is ordered
 *                                     futstate | means.  The mismatch is upstream's and is kept; `mean` and `cov` are returned
 *                                     too, so a caller who wants the aligned quadratic form can take it from those.
 *   totalbias  = mean over d of fcast[d, 1, w]   (`forecasts[:, 3]`: forecast_error of the first horizon); NaN when fcast is NULL.
 * out[w] holds HMCG_BIAS_STRIDE(K) doubles: uncbias, totalbias, mean[2K] (futstate | means), cov[2K][2K] (same order, symmetric,
 * both triangles written, bit-equal).  Draw arrays: the layouts and the nd_ld rule of the predictive entries; fcast is
 * (nd_ld, 2H, W).  HMCG_BIAS_ROUND5: every input is first rounded as a CSV cell is (as HMCG_PRED_ROUND5).
 * Second moments are taken about the window's draw 0 (S1_a = sum(v_a - p_a), S2_ab = sum (v_a - p_a)(v_b - p_b)), so a large
 * common offset costs no digits; cov_ab = (S2_ab - S1_a S1_b / nd) / (nd - 1).  nd = 1 gives a finite mean and NaN cov and
 * uncbias (0/0, as Statistics.cov).  NaN inputs propagate; nothing is special-cased.
 * Deterministic: draws are reduced in slabs of 1024 (the predictive entries' cut), inside a slab in an order that depends on
 * the draw index alone, the slabs in slab order, no floating-point atomics: bit-identical from run to run, from both entries
 * and for every chunking of the host entry's upload (HMCG_CHUNK_DRAWS under HMCG_DIAG=1).
 * Misuse (HMCG_E_BADARG, checked before any HIP call): struct_size, K outside 2..HMCG_MAXK, horizon outside 0..HMCG_PRED_MAXH,
 * W < 1, nd < 1, nd_ld < nd, a NULL mu / pi_end / out, NULL A with horizon > 0, fcast given with H outside 1..HMCG_MAXH. */
#define HMCG_BIAS_ROUND5 1
#define HMCG_BIAS_STRIDE(K) (2 + 2 * (K) + 4 * (K) * (K))
typedef struct hmcg_bias {
    int32_t struct_size, W, K, device;
    int64_t nd, nd_ld;                 /* draws per window; leading dimension of the draw arrays (>= nd) */
    int32_t horizon;                   /* 0..HMCG_PRED_MAXH; bias_calcs.jl uses 12 */
    int32_t H;                         /* fcast has 2H columns per window; 0 when fcast is NULL */
    int32_t flags, reserved;
} hmcg_bias;
/* Device entry: every data pointer is HBM-resident on p->device; enqueued on `stream` (NULL: the library's own) behind the
 * library's earlier work there; returns after enqueueing unless `timing` is given (kernel_ms: HIP events around the kernels). */
int hmcg_bias_moments_device(const hmcg_bias* p, const double* dmu, const double* dpi_end, const double* dA /* NULL iff horizon is 0 */,
                             const double* dfcast /* may be NULL */, double* dout /* [W][HMCG_BIAS_STRIDE(K)] */, void* stream,
                             hmcg_timing* timing);
/* Host entry (blocking): uploads the draws in chunks of whole slabs through pinned staging, the copy of one chunk beside the
 * kernel of the one before. */
int hmcg_bias_moments(const hmcg_bias* p, const double* mu, const double* pi_end, const double* A, const double* fcast, double* out,
                      hmcg_timing* timing);

/* ---- predictive mixture moments of the draws (skewness.jl, alt_forecasts.jl) -------------------------------------------------
 * The predictive law of window w at horizon h_j is the mixture of all nd * K components omega_{d,k} N(mu_{d,k}, sig2_{d,k}),
 * omega_d = pi_end_d * A_d^h_j (h_j successive row-vector x matrix products, k ascending in every dot product: the same bits as
 * the weights of hmcg_predictive_cdf and hmcg_bias_moments; horizons may come unsorted and repeated, equal horizons give equal
 * bits).  Its moments are draw sums of per-draw closed forms.  With s_d = sum_k omega_k, delta_k = mu_k - c, v_k = sig2_k and
 * the pivot c = the mixture mean of the window's draw 0 at that horizon:
 *   P0 = sum_d s_d                                    P1 = sum_d sum_k omega delta
 *   P2 = sum sum omega (delta^2 + v)                  P3 = sum sum omega delta (delta^2 + 3 v)
 *   P4 = sum sum omega (delta^4 + 6 delta^2 v + 3 v^2)
 * and per draw, normalised by s_d as skewness.jl:33 normalises p:  a_d = (sum_k omega delta) / s_d,  e_k = delta_k - a_d,
 *   var_d = sum omega (e^2 + v) / s_d,  skew_d = [sum omega e (e^2 + 3 v) / s_d] / (var_d sqrt(var_d)),  b_d = a_d - a_0:
 *   Q1 = sum b_d,  Q2 = sum b_d^2,  VW = sum var_d,  SK = sum skew_d.
 * out[w][j] holds HMCG_MIX_STRIDE doubles, m_i = P_i / P0:
 *   0 mean c + m1                        1 variance m2 - m1^2
 *   2 skewness (m3 - 3 m1 m2 + 2 m1^3) / variance^1.5
 *   3 excess kurtosis (m4 - 4 m1 m3 + 6 m1^2 m2 - 3 m1^4) / variance^2 - 3
 *   4 mean within-draw variance VW / nd  5 variance over the draws of the per-draw mean, Q2 / nd - (Q1 / nd)^2 (divisor nd)
 *   6 mean per-draw skewness SK / nd     7 mean weight P0 / nd
 * Draw arrays: the layouts and the nd_ld rule of the predictive entries.  HMCG_MIX_ROUND5: every input is first rounded as a CSV
 * cell is (as HMCG_PRED_ROUND5).  Nothing is special-cased: NaN propagates, a zero variance is v = 0, a zero pooled variance
 * gives NaN skewness and kurtosis (0/0).
 * Deterministic: draws are reduced in slabs of 1024 (the predictive entries' cut), inside a slab in an order that depends on
 * the draw index alone, the slabs in slab order, no floating-point atomics: bit-identical from run to run, from both entries
 * and for every chunking of the host entry's upload (HMCG_CHUNK_DRAWS under HMCG_DIAG=1).
 * Misuse (HMCG_E_BADARG, checked before any HIP call): struct_size, K outside 2..HMCG_MAXK, n_h outside 1..HMCG_MAXH, a horizon
 * outside 0..HMCG_PRED_MAXH, W < 1, nd < 1, nd_ld < nd, a NULL mu / sig2 / pi_end / out, NULL A with a horizon > 0. */
#define HMCG_MIX_ROUND5 1
#define HMCG_MIX_STRIDE 8
typedef struct hmcg_mixmom {
    int32_t struct_size, W, K, device;
    int64_t nd, nd_ld;                 /* draws per window; leading dimension of the draw arrays (>= nd) */
    int32_t n_h, flags;                /* horizons 1..HMCG_MAXH */
    int32_t horizons[HMCG_MAXH];       /* 0 = the end date itself (skewness.jl); alt_forecasts.jl uses 12 */
} hmcg_mixmom;
/* Device entry: every data pointer is HBM-resident on p->device; enqueued on `stream` (NULL: the library's own) behind the
 * library's earlier work there; returns after enqueueing unless `timing` is given (kernel_ms: HIP events around the kernels). */
int hmcg_mixture_moments_device(const hmcg_mixmom* p, const double* dmu, const double* dsig2, const double* dpi_end,
                                const double* dA /* NULL iff every horizon is 0 */, double* dout /* [W][n_h][HMCG_MIX_STRIDE] */,
                                void* stream, hmcg_timing* timing);
/* Host entry (blocking): uploads the draws in chunks of whole slabs through pinned staging, the copy of one chunk beside the
 * kernel of the one before. */
int hmcg_mixture_moments(const hmcg_mixmom* p, const double* mu, const double* sig2, const double* pi_end, const double* A,
                         double* out, hmcg_timing* timing);

/* ---- chain densities and running means of the draws (plots/mcplots.jl, plots/timeseriesplots.jl) ----------------------------
 * One generic entry over ONE draw array x of C columns per window, element (d, c, w) at d + nd_ld * (c + C * w): the layout of
 * mu, sig2 and pi_end with C = K, of A with C = K * K, of fcast with C = 2H.  Call it once per variable.
 * With x' = the value rounded as a CSV cell is under HMCG_DENS_ROUND5 (as HMCG_PRED_ROUND5) and x' = x otherwise, per window w
 * and column c:
 *   range[w][c][2] = (lo, hi): the caller's lo_hi[w][c][2] when lo_hi is given (the host entry wants them finite with hi >= lo;
 *     the device entry cannot look), else the minimum and maximum of the FINITE x' over all nd draws; both NaN with no finite value.
 *   counts[w][c][j][B + 3], int64, for the prefix d < cuts[j]: B bins, then `below`, `above`, `nan`.  The bin rule, in this
 *     order, every operation a rounded fp64 operation of its own (nothing fused):
 *       x' is NaN -> nan;  lo or hi is NaN -> below;  x' < lo (-inf too) -> below;  x' > hi (+inf too) -> above;
 *       !(hi > lo) -> bin 0;  else b = floor((x' - lo) * scale), scale = (double)B / (hi - lo), clamped to 0..B-1.
 *     The four groups of a prefix sum to cuts[j].
 *   stats[w][c][j][2] = mean and variance (divisor n - 1, n = cuts[j]) of x' over the prefix, both about the pivot p = x' of the
 *     window's draw 0:  a_d = x'_d - p, S1 = sum a_d, S2 = sum a_d^2, mean = p + S1 / n, variance = (S2 - S1 * S1 / n) / (n - 1).
 *     n = 1 gives a NaN variance; NaN and inf propagate into every prefix that holds them (a non-finite draw 0 into all); a column
 *     of identical values gives variance exactly 0.
 *   trace[w][c][i], i < trace_len: the mean of the first n_i = (i + 1) * trace_stride draws, p + (sum_{d < n_i} a_d) / n_i
 *     (plotchainmean: stride 1, length 10 000).
 * Deterministic: the draws are cut into pieces at every multiple of 1024 (the predictive entries' slabs) and at every cut; a
 * piece's float sums are taken in an order that depends on the draw's place in the piece alone, the pieces are added in piece
 * order; counts are integers.  No floating-point atomics: bit-identical from run to run, from both entries and for every
 * chunking of the host entry's upload (HMCG_CHUNK_DRAWS under HMCG_DIAG=1).
 * Misuse (HMCG_E_BADARG, checked before any HIP call): struct_size, W < 1, C outside 1..HMCG_MAXK^2, B outside
 * 1..HMCG_DENS_MAXBINS, nd < 1 or > 2^53 (n must be an exact fp64 divisor; the counters are 64-bit), nd_ld < nd, n_cuts outside
 * 1..HMCG_MAXH, a cut outside 1..nd or not above the one before, trace_len outside 0..HMCG_DENS_MAXTRACE, trace_stride < 1,
 * trace_len * trace_stride > nd, more than 2^31 - 1 blocks in one launch (W * pieces * column groups, or W * C), a NULL x / range / counts / stats, NULL trace with
 * trace_len > 0, and on the host entry a lo_hi pair that is not finite or has hi < lo. */
#define HMCG_DENS_ROUND5 1
#define HMCG_DENS_MAXBINS 512
#define HMCG_DENS_MAXTRACE 65536
typedef struct hmcg_density {
    int32_t struct_size, W, C, device;
    int64_t nd, nd_ld;                 /* draws per window; leading dimension of the draw array (>= nd) */
    int32_t B, n_cuts;                 /* bins 1..HMCG_DENS_MAXBINS; prefixes 1..HMCG_MAXH */
    int64_t cuts[HMCG_MAXH];           /* strictly ascending prefix lengths, 1..nd (mcplots.jl: 100000, 150000, 200000, 250000) */
    int32_t trace_len, flags;          /* running-mean points 0..HMCG_DENS_MAXTRACE; HMCG_DENS_ROUND5 */
    int64_t trace_stride;              /* >= 1, trace_len * trace_stride <= nd */
} hmcg_density;
/* Device entry: every data pointer is HBM-resident on p->device; enqueued on `stream` (NULL: the library's own) behind the
 * library's earlier work there; returns after enqueueing unless `timing` is given (kernel_ms: HIP events around the kernels). */
int hmcg_chain_density_device(const hmcg_density* p, const double* dx, const double* dlo_hi /* [W][C][2] or NULL */,
                              double* drange /* [W][C][2] */, int64_t* dcounts /* [W][C][n_cuts][B + 3] */,
                              double* dstats /* [W][C][n_cuts][2] */, double* dtrace /* [W][C][trace_len]; NULL iff trace_len == 0 */,
                              void* stream, hmcg_timing* timing);
/* Host entry (blocking): uploads the draws in chunks of whole slabs through pinned staging, the copy of one chunk beside the
 * kernel of the one before -- twice with lo_hi NULL (the range, then the counts), once with lo_hi given. */
int hmcg_chain_density(const hmcg_density* p, const double* x, const double* lo_hi, double* range, int64_t* counts, double* stats,
                       double* trace, hmcg_timing* timing);

/* ---- autocorrelation, effective sample size and split-R-hat of the draws ----------------------------------------------------
 * One generic entry over ONE draw array x of C columns per window, in the layout of hmcg_chain_density: element (d, c, w) at
 * d + nd_ld * (c + C * w).  With x' = the value rounded as a CSV cell is under HMCG_ACF_ROUND5 and x' = x otherwise, n = nd,
 * p = x' of the window's draw 0 and a_d = x'_d - p (one rounded fp64 subtraction), per window w and column c:
 *   S1 = sum a_d, S2 = sum a_d^2, m = S1 / n, mean = p + m, variance = (S2 - S1 * S1 / n) / (n - 1)  (density's `stats`).
 *   C_l = sum_{d = l}^{n - 1} a_d a_{d - l}, l = 0..L;  H_l = a_0 + .. + a_{l - 1},  T_l = a_{n - 1} + .. + a_{n - l}
 *   (running sums in l, H_0 = T_0 = 0).
 *   acov[w][c][l] = (C_l - m (2 S1 - H_l - T_l) + (n - l) m m) / n: the biased autocovariance about the sample mean, exact in
 *     the pivoted form.  Operation order, every step a rounded fp64 operation of its own:
 *       q = ((2 S1) - H_l) - T_l;  r = C_l - m q;  s = ((double)(n - l) * m) * m;  acov_l = (r + s) / n.
 *   From acov, likewise one rounded operation per step, nothing fused (this part is ABI; tests restate it in numpy and compare bits):
 *     !(acov_0 > 0): tau, ess, mcse NaN, pairs = 0, truncated = 0.  Else rho_l = acov_l / acov_0 and Geyer's initial monotone
 *     sequence over (L + 1) / 2 pairs: tau = -1, prev = +inf; for k = 0, 1, ..: P = rho_2k + rho_2k+1; stop if !(P > 0);
 *     if P > prev then P = prev; tau = tau + 2 P; prev = P.  pairs = the pairs used; truncated = 1 when every pair was used
 *     and none stopped the sequence (the lag window is too short), else 0 (L = 0 has no pair at all: truncated = 1); pairs = 0 with acov_0 > 0 gives tau NaN.
 *     ess = n / tau;  mcse = sqrt((variance * tau) / n).
 *   Split-R-hat of the single chain: h = n / 2 (integer), halves [0, h) and [n - h, n), S1 and S2 of each half about p:
 *     m_i = S1_i / h, v_i = (S2_i - S1_i * S1_i / h) / (h - 1), Wv = (v1 + v2) / 2,
 *     varplus = (((h - 1) / h) * Wv + ((m1 - m2) * (m1 - m2)) / 2) + (S1_mid - S1_mid), rhat = sqrt(varplus / Wv).  S1_mid is the
 *     draw between the halves of an odd n (0 for an even n): the last term is 0 unless that draw is not finite, which then
 *     reaches rhat as it reaches every other output.  Nothing is special-cased: h < 2 or a constant column gives NaN by 0 / 0.
 *   diag[w][c][HMCG_ACF_STRIDE] = mean, variance, tau, ess, mcse, pairs, truncated, rhat (pairs and truncated as doubles).
 * NaN or inf anywhere in a column makes every output of that column NaN or inf (acov: NaN), pairs = truncated = 0.
 * Deterministic: a product (d, d - l) belongs to the 1024-draw slab of d; a slab's sum per lag is taken in an order fixed by
 * the place in the slab and L, the slab sums are added in ascending slab order into running accumulators; S1 and S2 are
 * taken per slab and per third of the chain ([0, h), [h, n - h), [n - h, n)) by a fixed butterfly with unfused squares, the
 * slabs added in order, S1 = (first + middle) + second.  No floating-point atomics: bit-identical from run to run, from both entries and for every
 * chunking of the host entry's upload (HMCG_CHUNK_DRAWS under HMCG_DIAG=1).
 * Misuse (HMCG_E_BADARG, checked before any HIP call): struct_size, W < 1, C outside 1..HMCG_MAXK^2, nd < 1 or > 2^53,
 * nd_ld < nd, L outside 0..HMCG_ACF_MAXLAG, L > nd - 1, W * C above 2^31 - 1 blocks, a NULL x / acov / diag. */
#define HMCG_ACF_ROUND5 1
#define HMCG_ACF_MAXLAG 1024
#define HMCG_ACF_STRIDE 8
typedef struct hmcg_autocorr {
    int32_t struct_size, W, C, device;
    int64_t nd, nd_ld;                 /* draws per window; leading dimension of the draw array (>= nd) */
    int32_t L, flags;                  /* largest lag 0..min(HMCG_ACF_MAXLAG, nd - 1); HMCG_ACF_ROUND5 */
} hmcg_autocorr;
/* Device entry: every data pointer is HBM-resident on p->device; enqueued on `stream` (NULL: the library's own) behind the
 * library's earlier work there; returns after enqueueing unless `timing` is given (kernel_ms: HIP events around the kernels). */
int hmcg_chain_autocorr_device(const hmcg_autocorr* p, const double* dx, double* dacov /* [W][C][L + 1] */,
                               double* ddiag /* [W][C][HMCG_ACF_STRIDE] */, void* stream, hmcg_timing* timing);
/* Host entry (blocking): uploads the draws once in chunks of whole slabs through pinned staging, each chunk with the
 * min(L, d0) draws before it in front, the copy of one chunk beside the kernel of the one before. */
int hmcg_chain_autocorr(const hmcg_autocorr* p, const double* x, double* acov, double* diag, hmcg_timing* timing);

/* ---- per-draw CSV output (host code, no GPU): basicsave / saveresults, src/Hmc.jl:707-748 ------------------------------
 * The five per-window files `filtered_means_<date>.csv`, `filtered_variances_<date>.csv`, `filtered_state_probs_<date>.csv`,
 * `filtered_trans_probs_<date>.csv`, `forecasts_<date>.csv` (:741-746), written straight from the draw arrays of the
 * estimate entries above (window w's block of every array), byte for byte as upstream's CSV.jl 0.5.16 writes them: header
 * `date[,signalid],state_1..K | trans_i_j (i fastest, :727) | forecast_h,forecast_error_h [,signal_1..]`, one row per kept
 * draw, values round(x; digits=5) (:719), LF line ends, CSV.jl float text (shortest round-trip digits; integral values
 * without a fraction; |x| < 1e-4 as <integer mantissa>e-<n>).  250 000 rows x 5 files per window in production
 * (code/run_hmm.jl:103-104).  Any of mu/sig2/pi_end/A/fcast may be NULL (that file is not written).
 * dates: W strings "yyyy-mm-dd" (the end date of each window, Hmc.enddate).  sigvals (signal path, [W][n_samples][nsave_ld])
 * adds the `signalid` column (1-based sample number of the row) and the `signal_j` columns (:715-717).
 * n_threads: windows are written in parallel (0 = one thread per hardware thread).  Returns 0 or HMCG_E_BADARG (bad
 * arguments / a file could not be written). */
#define HMCG_CSV_LEGACY_TRANS_HEADER 1 /* name the transition columns trans_<j>_<i> as the committed fixtures do
                                          (code/deprecated/Hmc.jl_08072019bak:711); data order is unchanged */
int hmcg_save_results_csv(const char* dir, int32_t W, const char* const* dates, int32_t K, int32_t H, const int32_t* horizons,
                          int64_t nd, const double* mu, const double* sig2, const double* pi_end, const double* A,
                          const double* fcast, const double* sigvals, int32_t n_samples, int32_t nsave, int32_t nsave_ld,
                          int32_t flags, int32_t n_threads);
/* One table: `date,<colnames>` with n rows from a column-major block (element (d, c) at data[d + ld*c]), rounded to
 * `precision` digits (basicsave, :707-722). */
int hmcg_write_table_csv(const char* path, const char* date, int32_t ncol, const char* const* colnames, const double* data,
                         int64_t n, int64_t ld, int32_t precision);
/* CSV.jl 0.5.16 text of one Float64 into buf (>= 48 bytes, NUL-terminated); returns its length. */
int hmcg_format_float(double x, char* buf);

#ifdef __cplusplus
}
#endif
#endif /* HMCG_H */
