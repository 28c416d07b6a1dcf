/* hmcg_ergodic.h -- the h -> infinity limit of the draw statistics: the companion header of hmcg.h.
 *
 * hmcg.h is closed at HMCG_VERSION 109 (see hmcg_order.h and DESIGN.md section 9); this header includes it and leaves it as it
 * is.  Both entries below are exported from libhmcgibbs.so.
 */
#ifndef HMCG_ERGODIC_H
#define HMCG_ERGODIC_H
#include "hmcg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ergodic regime law, expected durations and long-run moments of the draws ----------------------------------------------
 * Inputs in the layouts of the predictive entries: mu and sig2, element (d, k, w) at d + nd_ld * (k + K * w); A, element
 * (d, i, j, w) at d + nd_ld * (i + K * (j + K * w)), row i the from-state.  Draws d >= nd (the padding) are never read.  Under
 * HMCG_ERG_ROUND5 every input is first rounded as a CSV cell (rint(x * 1e5) / 1e5 correctly rounded, a zero quotient with the
 * sign of x, the value itself where the quotient is not finite).
 * THE DIAGONAL OF A IS NEVER READ: the law computed is that of the chain whose off-diagonal transition weights are the
 * off-diagonal cells, which is well defined when rounded rows do not sum to one.
 *
 * Per draw, C = HMCG_ERG_COLS(K) values; every step ONE rounded fp64 operation, nothing fused, in the stated order (this part
 * is ABI; tests restate it).  A sum "a_0 + .. + a_n" starts at a_0 and adds the terms in the order written.
 *   c = 0..K-1     pi, the stationary law, by the Grassmann-Taksar-Heyman elimination on a copy P of the off-diagonal cells:
 *                    for n = K-1 down to 1:  S = P[n][0] + .. + P[n][n-1];
 *                                            P[i][n] = P[i][n] / S                        for i < n;
 *                                            P[i][j] = P[i][j] + P[i][n] * P[n][j]        for i, j < n, i != j;
 *                    x[0] = 1;  x[j] = x[0] * P[0][j] + .. + x[j-1] * P[j-1][j]           for j = 1..K-1;
 *                    tot = x[0] + .. + x[K-1];  pi[k] = x[k] / tot.
 *                  No subtraction anywhere.  Nothing is special-cased: a reducible draw (S == 0) yields the inf / NaN that IEEE
 *                  gives, a transient state an exact 0.
 *   c = K..2K-1    dur[i] = 1 / (sum over j != i of A[i][j], j ascending), the expected duration of regime i: 1 / (1 - A_ii) of
 *                  a stochastic row without its cancellation; +inf for an absorbing state.
 *   c = 2K         m = pi[0] * mu[0] + .. + pi[K-1] * mu[K-1], the long-run mean.
 *   c = 2K + 1     v = within + between, the long-run variance: within = pi[0] * sig2[0] + .. + pi[K-1] * sig2[K-1],
 *                  between = t_0 + .. + t_{K-1}, t_k = pi[k] * (e_k * e_k), e_k = mu[k] - m.  No E[y^2] - m^2.
 * cols (may be NULL), element (d, c, w) at d + nd_ld * (c + C * w): the layout of hmcg_chain_density / hmcg_chain_quantiles /
 * hmcg_chain_autocorr, so cols can be handed to them as it is.
 *
 * Pooled over the draws: a draw is GOOD when all C of its values are finite.  n[w] = (good, nd - good).
 * out[w][c][2] = (mean, variance) of column c over the good draws, divisor good - 1; good = 1 gives a NaN variance, good = 0 NaNs.
 * Second moments are taken about the pivot p_c = column c of the window's draw 0 when that draw is good, 0.0 otherwise:
 *   mean = p_c + S1 / good,  variance = (S2 - S1 * S1 / good) / (good - 1),  S1 = sum (x - p_c),  S2 = sum (x - p_c)^2.
 * Deterministic: slabs of 1024 draws as in the predictive entries, a draw's place inside a slab depends on the draw index
 * alone, the slabs are added in slab order, no floating-point atomics.  Results are bit-identical from run to run, from both
 * entries, with and without cols, and for every HMCG_CHUNK_DRAWS under HMCG_DIAG=1.
 * Misuse (HMCG_E_BADARG, checked before any HIP call, in this order): struct_size, K outside 2..HMCG_MAXK, W < 1, nd < 1,
 * nd_ld < nd, a NULL mu / sig2 / A / out / n. */
#define HMCG_ERG_ROUND5 1
#define HMCG_ERG_COLS(K) (2 * (K) + 2)
typedef struct hmcg_ergodic {
    int32_t struct_size, W, K, device;
    int64_t nd, nd_ld;                /* draws per window; leading dimension of the draw arrays and of cols (>= nd) */
    int32_t flags, reserved;          /* HMCG_ERG_ROUND5 */
} hmcg_ergodic;                       /* 40 bytes */
/* Device entry: every data pointer is HBM-resident on p->device; enqueued on `stream` (NULL: the library's own) behind the
 * library's earlier work there; returns after enqueueing unless `timing` is given (kernel_ms: HIP events around the kernels). */
int hmcg_ergodic_moments_device(const hmcg_ergodic* p, const double* dmu, const double* dsig2, const double* dA,
                                double* dcols /* [W][C][nd_ld], may be NULL */, double* dout /* [W][C][2] */,
                                int64_t* dn /* [W][2] */, void* stream, hmcg_timing* timing);
/* Host entry (blocking): one pass of the upload ring of the predictive entries; cols, when given, comes back chunk by chunk
 * (its copies are then inside kernel_ms). */
int hmcg_ergodic_moments(const hmcg_ergodic* p, const double* mu, const double* sig2, const double* A, double* cols /* may be NULL */,
                         double* out, int64_t* n, hmcg_timing* timing);

#ifdef __cplusplus
}
#endif
#endif /* HMCG_ERGODIC_H */
