/* hmcg_fan.h -- quantiles of the predictive regime mixture (median, forecast bands, value at risk): a companion header of hmcg.h.
 *
 * hmcg.h is closed at HMCG_VERSION 109 (see hmcg_order.h and DESIGN.md section 9); this header includes it and leaves it as it
 * is.  Both entries below are exported from libhmcgibbs.so.
 */
#ifndef HMCG_FAN_H
#define HMCG_FAN_H
#include "hmcg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- predictive quantiles of the regime mixture: the fan chart -------------------------------------------------------------
 * The predictive law of window w at horizon h is the mixture of nd * K normals whose CDF hmcg_predictive_cdf evaluates:
 *   F(y) = mean over the draws d < nd of  sum_k omega_d[k] * Phi((y - mu_dk) * c_dk),
 *   omega_d = pi_end_d A_d^h (h successive row-vector x matrix products, k ascending in every dot product),
 *   c = 1 / (1.4142135623730951 * sqrt(sig2)),  Phi(t) = 0.5 * erfc(-t),
 *   the sum over k: w_0 * ph_0 for k = 0, then fma(w_k, ph_k, F);  the draws added in draw order inside a slab of 1024 draws,
 *   the slab sums added in slab order, the total divided by nd.
 * That is the expression and the order of hmcg_predictive_cdf: without HMCG_FAN_ROUND5 an F computed here is bit-equal to what
 * that entry returns for the same point.  These entries invert F at the probabilities probs[i].
 *
 * Inputs in the layouts and under the nd_ld rule of the predictive entries: mu, sig2, pi_end element (d, k, w) at
 * d + nd_ld * (k + K * w); A element (d, i, j, w) at d + nd_ld * (i + K * (j + K * w)), row i the from-state; A may be NULL if and
 * only if every horizon is 0.  Draws d >= nd are never read.  Under HMCG_FAN_ROUND5 every draw input is first rounded as a CSV
 * cell (rint(x * 1e5) / 1e5 correctly rounded, a zero quotient with the sign of x, the value itself where the quotient is not
 * finite).  Evaluation points are never rounded.
 *
 * The algorithm is ABI.  Every step below is ONE rounded fp64 operation, nothing fused, in the order written.
 *   points of a bracket (lo, hi) cut into M cells:  step = (hi - lo) / M;  y_m = lo + m * step for m < M,  y_M = hi.
 *   1. range pass, once per window (not per horizon): sd = sqrt(sig2);  lo0 = fmin over d < nd, k of (mu - 40 * sd),
 *      hi0 = fmax of (mu + 40 * sd); fmin / fmax ignore NaN (all NaN: NaN).  At |z| >= 40 Phi is exactly 0 or 1.
 *   2. round 1, per (w, j): M = 128 over (lo0, hi0); all 129 F(y_m) are evaluated once and serve every probability.
 *   3. rounds 2..R, per (w, j, i): M = 32 over the item's bracket; the 31 interior points are evaluated, F at the two ends is
 *      carried over from the round before.
 *   4. cell choice, every round, per (w, j, i): m* = the smallest m in 1..M with F(y_m) >= p, M if there is none (a NaN
 *      compares false); the new (lo, hi, Flo, Fhi) = (y_{m*-1}, y_{m*}, F_{m*-1}, F_{m*}).
 *   5. finish: Flo or Fhi NaN: q = NaN, flag 1;  else !(Fhi - Flo > 0): q = lo, flag 4;  else p > Fhi: q = hi, flag 2;
 *      else q = lo + (hi - lo) * ((p - Flo) / (Fhi - Flo)).
 * Nothing else is special-cased: zero variances, infinite means and lo0 == hi0 give what IEEE gives, as in the CDF entry.
 *
 * out[w][j][i][5] = (q, lo, hi, Flo, Fhi): the quantile, the last bracket and the computed CDF at its ends.
 * range[w][2] = (lo0, hi0).   flag[w][j][i]: HMCG_FAN_NAN | HMCG_FAN_UNREACHED | HMCG_FAN_FLAT, at most one of them.
 * A p that no F reaches (rounded weights that sum below it) sends every round to its last cell.  Phi is exactly 1 from some
 * 8.3 standard deviations above a mean, so once that cell lies above every component F is flat on it and the flag is
 * HMCG_FAN_FLAT (rule 5 tests the flat cell first); HMCG_FAN_UNREACHED is what such a p gets while the last cell still climbs.
 * The launch count depends on `rounds` alone (2 + 2 R on the device entry); nothing is read back between the rounds.
 * Deterministic: no atomics; results are bit-identical from run to run, from both entries, and for every HMCG_CHUNK_DRAWS under
 * HMCG_DIAG=1.  Equal horizons give equal bits.
 * Misuse (HMCG_E_BADARG, checked before any HIP call, in this order): struct_size, K outside 2..HMCG_MAXK, W < 1, n_h outside
 * 1..HMCG_MAXH, a horizon outside 0..HMCG_PRED_MAXH, n_p outside 1..HMCG_FAN_MAXP, a probability not finite or not strictly
 * inside (0, 1), rounds outside 0..HMCG_FAN_MAXROUNDS, nd < 1, nd_ld < nd, a NULL mu / sig2 / pi_end / out / range / flag, a NULL
 * A with a horizon > 0. */
#define HMCG_FAN_ROUND5 1
#define HMCG_FAN_MAXP 16
#define HMCG_FAN_MAXROUNDS 10
#define HMCG_FAN_ROUNDS_DEFAULT 4
#define HMCG_FAN_STRIDE 5             /* doubles per (window, horizon, probability) of out */
#define HMCG_FAN_NAN 1
#define HMCG_FAN_UNREACHED 2
#define HMCG_FAN_FLAT 4
typedef struct hmcg_fan {
    int32_t struct_size, W, K, device;
    int64_t nd, nd_ld;                /* draws per window; leading dimension of the draw arrays (>= nd) */
    int32_t n_h, n_p;
    int32_t horizons[HMCG_MAXH];      /* 0..HMCG_PRED_MAXH, in any order, repeats allowed */
    int32_t rounds, flags;            /* 1..HMCG_FAN_MAXROUNDS, 0: HMCG_FAN_ROUNDS_DEFAULT;  HMCG_FAN_ROUND5 */
    double probs[HMCG_FAN_MAXP];      /* strictly inside (0, 1); carried here: no device pointer for them */
    int64_t reserved;
} hmcg_fan;                           /* 216 bytes */
/* Device entry: every data pointer is HBM-resident on p->device; enqueued on `stream` (NULL: the library's own) behind the
 * library's earlier work there; returns after enqueueing unless `timing` is given (kernel_ms: HIP events around the kernels). */
int hmcg_predictive_quantiles_device(const hmcg_fan* p, const double* dmu, const double* dsig2, const double* dpi_end, const double* dA,
                                     double* dout /* [W][n_h][n_p][5] */, double* drange /* [W][2] */,
                                     int32_t* dflag /* [W][n_h][n_p] */, void* stream, hmcg_timing* timing);
/* Host entry (blocking): R + 1 passes of the upload ring of the predictive entries, one for the range and one per round. */
int hmcg_predictive_quantiles(const hmcg_fan* p, const double* mu, const double* sig2, const double* pi_end, const double* A,
                              double* out, double* range, int32_t* flag, hmcg_timing* timing);

#ifdef __cplusplus
}
#endif
#endif /* HMCG_FAN_H */
