/* hmcg_order.h -- order statistics of the draws: the companion header of hmcg.h.
 *
 * hmcg.h is closed at HMCG_VERSION 109: its declarations, and the tables that mirror them, are pinned by tests.  What the
 * library gains from here on is declared in companion headers like this one, which include hmcg.h and leave it as it is
 * (DESIGN.md section 9).  Both entries below are exported from libhmcgibbs.so.
 */
#ifndef HMCG_ORDER_H
#define HMCG_ORDER_H
#include "hmcg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- exact quantiles and credible limits of the draws ------------------------------------------------------------------------
 * One generic entry over ONE draw array x of C columns per window, in the layout of hmcg_chain_density: element (d, c, w) at
 * d + nd_ld * (c + C * w); draws d >= nd (the padding) are never read.  x' = the value rounded as a CSV cell is under
 * HMCG_ORD_ROUND5 (rint(x * 1e5) / 1e5 correctly rounded, a zero quotient with the sign of x, the value itself where the
 * quotient is not finite) and x' = x otherwise.  Per window w and column c:
 *   n[w][c] = (m, nan): m = the draws whose x' is not NaN, nan = the rest; m + nan = nd.
 *   The m values are ranked by the IEEE total order restricted to non-NaN values, -inf < .. < -0.0 < +0.0 < .. < +inf:
 *   x_(0) <= .. <= x_(m-1).  Infinities are ranked like any value.
 *   Per probability p = probs[i], every step ONE rounded fp64 operation, nothing fused (this part is ABI; tests restate it):
 *     h = p * (double)(m - 1);  j = (int64)floor(h);  g = h - (double)j;  lo = x_(j);  hi = x_(min(j + 1, m - 1));
 *     value = lo when g == 0 or lo == hi; otherwise v = lo + g * (hi - lo) and value = v > hi ? hi : v
 *   (Julia's / numpy's default, type 7, with a fixed operation order; lo = -inf with g > 0 gives NaN by the rule).
 *   q[w][c][i][HMCG_ORD_STRIDE] = value, lo, hi, g.  m == 0 gives four NaNs.
 * lo and hi are BIT COPIES of elements of x' -- a selection, not an estimate.
 * Deterministic: the selection is a radix selection on the order-preserving 64-bit key of x' (csrc/order_plan.hpp) and counts
 * integers only (LDS and global integer atomics commute); there is no floating-point accumulation anywhere.  Results are
 * bit-identical from run to run, from both entries and for every grouping of the host entry's upload (HMCG_CHUNK_COLS under
 * HMCG_DIAG=1).  The counters are 32-bit, hence HMCG_ORD_MAXND.
 * Misuse (HMCG_E_BADARG, checked before any HIP call, in this order): struct_size, W < 1, C outside 1..HMCG_MAXK^2, nd < 1,
 * nd > HMCG_ORD_MAXND, nd_ld < nd, Q outside 1..HMCG_ORD_MAXQ, a probability that is NaN or outside [0, 1], W * C above
 * 2^31 - 1 blocks, a NULL x / q / n. */
#define HMCG_ORD_ROUND5 1
#define HMCG_ORD_MAXQ   16
#define HMCG_ORD_STRIDE 4
#define HMCG_ORD_MAXND  2147483647LL
typedef struct hmcg_quantiles {
    int32_t struct_size, W, C, device;
    int64_t nd, nd_ld;                /* draws per window; leading dimension of the draw array (>= nd) */
    int32_t Q, flags;                 /* 1..HMCG_ORD_MAXQ probabilities; HMCG_ORD_ROUND5 */
    double  probs[HMCG_ORD_MAXQ];     /* each finite, 0 <= p <= 1; any order, repeats allowed */
} hmcg_quantiles;                     /* 168 bytes */
/* Device entry: every data pointer is HBM-resident on p->device; enqueued on `stream` (NULL: the library's own) behind the
 * library's earlier work there; returns after enqueueing unless `timing` is given (kernel_ms: HIP events around the kernel). */
int hmcg_chain_quantiles_device(const hmcg_quantiles* p, const double* dx, double* dq /* [W][C][Q][HMCG_ORD_STRIDE] */,
                                int64_t* dn /* [W][C][2] */, void* stream, hmcg_timing* timing);
/* Host entry (blocking): a selection needs its whole column resident, so the draws go up in groups of WHOLE COLUMNS through
 * pinned staging, the copy of one group beside the kernel of the one before. */
int hmcg_chain_quantiles(const hmcg_quantiles* p, const double* x, double* q, int64_t* n, hmcg_timing* timing);

#ifdef __cplusplus
}
#endif
#endif /* HMCG_ORDER_H */
