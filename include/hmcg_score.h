/* hmcg_score.h -- proper scores of the predictive regime mixture against the realised value (CRPS, PIT, density): a companion
 * header of hmcg.h.
 *
 * hmcg.h is closed at HMCG_VERSION 109 (see hmcg_order.h and DESIGN.md section 9); this header includes it and leaves it as it
 * is.  Both entries below are exported from libhmcgibbs.so.
 */
#ifndef HMCG_SCORE_H
#define HMCG_SCORE_H
#include "hmcg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- scores of the predictive regime mixture --------------------------------------------------------------------------------
 * Inputs in the layouts and under the nd_ld rule of the predictive entries: mu, sig2, pi_end element (d, k, w) at
 * d + nd_ld * (k + K * w); A element (d, i, j, w) at d + nd_ld * (i + K * (j + K * w)), row i the from-state; A may be NULL if and
 * only if every horizon is 0.  Draws d >= nd are never read.  yreal[n_h][W] (the (H, W) layout of hmcg.h): the realised value of
 * window w at horizons[j] at j * W + w, NaN for unknown; never rounded.  Under HMCG_SCORE_ROUND5 every draw input is first rounded
 * as a CSV cell (rint(x * 1e5) / 1e5 correctly rounded, a zero quotient with the sign of x, the value itself where the quotient
 * is not finite), as under HMCG_FAN_ROUND5.
 *
 * Thinning: a call uses the draws d = u * stride, u = 0 .. n_u - 1, n_u = ceil(nd / stride).  stride = 0 asks for the default,
 * the smallest stride with n_u <= HMCG_SCORE_DRAWS_DEFAULT (stride = ceil(nd / 4096); nd = 250 000: stride 62, n_u = 4 033).
 * stride = 1 is the exact score over every draw.  Cost: N = n_u * K components, N^2 / 2 + 128 N pair terms per window (the
 * symmetric half of the component square in tiles of 256), each one erf, one exp, one square root and one division in fp64, and
 * shared by all horizons.
 *
 * The law of window w at horizon h is the mixture of the N normals N(mu_uk, sig2_uk) with the weights omega_uk / n_u,
 * omega_u = pi_end_u A_u^h (h successive row-vector x matrix products, k ascending in every dot product: the bits of the
 * predictive entries).  Component c = u * K + k.
 *
 * out[w][j][5] = (crps, e_abs, e_pair, pit, pdf) for y = yreal[j][w]:
 *   e_abs  = E|X - y|  = (1 / n_u)   sum_c omega_c a(y - mu_c, sig2_c)
 *   e_pair = E|X - X'| = (1 / n_u^2) sum_c sum_c' omega_c omega_c' a(mu_c - mu_c', sig2_c + sig2_c'), the diagonal included
 *   crps   = e_abs - 0.5 * e_pair
 *   pit    = F(y), pdf = F'(y) of the mixture.
 * A NaN y makes crps, e_abs, pit and pdf of that item NaN; e_pair (the Gini mean difference of the forecast) does not depend on y.
 *
 * The algorithm is ABI.  Every step below is ONE rounded fp64 operation, nothing fused unless fma is written, in the order written.
 *   a(m, S2):  S2 == 0: |m|.  Otherwise  s = sqrt(S2);  r = 1 / (1.4142135623730951 * s);  t = m * r;  e = erf(t);
 *     g = exp(-(t * t));  a = (m * e) + ((s * 0.7978845608028654) * g).  The zero variance is the one special case (it removes the
 *     0 / 0 of m = 0); a negative or NaN variance gives what IEEE gives.
 *   per used draw u and horizon j (the linear pass), with y = yreal[j][w], over k ascending:
 *     c = 1 / (1.4142135623730951 * sqrt(sig2));  t = (y - mu) * c;  ph = 0.5 * erfc(-t);  ak = a(y - mu, sig2);
 *     dk = (c * 0.5641895835477563) * exp(-(t * t))      (a zero variance: what IEEE gives)
 *     F = w_0 * ph_0, then fma(w_k, ph_k, F);  E and P likewise from ak and dk.
 *   F, E, P are added in draw order inside a slab of 1024 used draws (from 0.0), the slab sums in slab order (from 0.0), and
 *   pit = sum F / n_u, e_abs = sum E / n_u, pdf = sum P / n_u.  That is the expression and the order of hmcg_predictive_cdf over
 *   the used draws: with stride = 1 and without HMCG_SCORE_ROUND5, pit is bit-equal to what that entry returns at y.
 *   Longest chain of additions a term of e_abs passes through: L1 = (K - 1) + 1024 + ceil(n_u / 1024).
 *   the pair pass: the components are cut into nT = ceil(N / 256) tiles of 256.  Block b < ceil(nT / 2) takes the rows of tiles
 *   r = b and then r = nT - 1 - b (once if they are equal).  Thread t of the block holds, per horizon, off = 0.0 and diag = 0.0;
 *   for each of its rows, with i = 256 r + t < N:  for c = 0 .. 256 r - 1 ascending:  off += (w_i * w_c) * a(mu_i - mu_c, sig2_i +
 *   sig2_c);  for c = 256 r .. min(256 r + 256, N) - 1 ascending:  diag += the same term.  Its value v = (off + off) + diag (0.0 for
 *   a thread without a component).  The 64 values of a wave are added by the butterfly xor 32, 16, .. 1 (x += x of lane ^ m), the
 *   four waves in wave order from wave 0's sum: one partial per (window, block, horizon).
 *   finish: S = the partials added in block order from 0.0;  e_pair = S / (n_u * n_u)  (the product in fp64, one division);
 *   crps = e_abs - (0.5 * e_pair).
 *   Longest chain of a term of e_pair: L2 = N + 2 + 6 + 3 + ceil(nT / 2).
 * No atomics; results are bit-identical from run to run, from both entries, and for every grouping of windows the host entry
 * uploads (HMCG_SCORE_GROUP_WINDOWS under HMCG_DIAG=1 caps the windows of a group).  Equal horizons give equal bits.
 * Misuse (HMCG_E_BADARG, checked before any HIP call, in this order): struct_size, K outside 2..HMCG_MAXK, W < 1, n_h outside
 * 1..HMCG_MAXH, a horizon outside 0..HMCG_PRED_MAXH, nd < 1, nd_ld < nd, stride < 0, a block count past one launch (2^31 - 1), a
 * NULL mu / sig2 / pi_end / yreal / out, a NULL A with a horizon > 0. */
#define HMCG_SCORE_ROUND5 1
#define HMCG_SCORE_DRAWS_DEFAULT 4096
#define HMCG_SCORE_STRIDE 5           /* doubles per (window, horizon) of out */
typedef struct hmcg_score {
    int32_t struct_size, W, K, device;
    int64_t nd, nd_ld;                /* draws per window; leading dimension of the draw arrays (>= nd) */
    int32_t n_h, flags;               /* HMCG_SCORE_ROUND5 */
    int32_t horizons[HMCG_MAXH];      /* 0..HMCG_PRED_MAXH, in any order, repeats allowed */
    int64_t stride;                   /* every stride-th draw is used; 0: the default thinning */
    int64_t reserved;
} hmcg_score;                         /* 88 bytes */
/* Device entry: every data pointer is HBM-resident on p->device; enqueued on `stream` (NULL: the library's own) behind the
 * library's earlier work there; returns after enqueueing unless `timing` is given (kernel_ms: HIP events around the kernels). */
int hmcg_predictive_scores_device(const hmcg_score* p, const double* dmu, const double* dsig2, const double* dpi_end, const double* dA,
                                  const double* dyreal /* [n_h][W] */, double* dout /* [W][n_h][5] */, void* stream, hmcg_timing* timing);
/* Host entry (blocking): reads only the used draws, stages them compactly and uploads the windows in groups. */
int hmcg_predictive_scores(const hmcg_score* p, const double* mu, const double* sig2, const double* pi_end, const double* A,
                           const double* yreal, double* out, hmcg_timing* timing);

#ifdef __cplusplus
}
#endif
#endif /* HMCG_SCORE_H */
