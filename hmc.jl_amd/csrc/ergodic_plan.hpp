// ergodic_plan.hpp -- the argument rules of hmcg_ergodic_moments[_device], the size of its work area and the per-draw
// arithmetic (stationary law by GTH, durations, long-run mean and variance).  Plain C++17 without a HIP header (in the manner
// of order_plan.hpp): a g++-compiled program runs exactly the code the library runs, on the CPU; the kernel of ergodic.hip
// expands the same erg_draw, so the two compile the same statements.
//
// Why GTH: a posterior draw of a persistent chain is nearly reducible (A_ii = 0.99999) and, as a row of rounded CSV cells, no
// longer sums to one.  Solving (A' - I | 1) loses 1 / (1 - A_ii) of its accuracy to the cancellation in A_ii - 1; the
// Grassmann-Taksar-Heyman elimination never forms that difference -- the pivot is the sum of the row's off-diagonal cells --
// and every intermediate is a sum, product or quotient of non-negative numbers (tests/ergodic_cases.py counts the roundings).
#pragma once
#include <cstdint>
#include <cstdio>

#include "../../include/hmcg_ergodic.h"
#include "stat_plan.hpp"

#ifdef __HIPCC__
#define HMCG_ERG_HD __host__ __device__ __forceinline__
#else
#define HMCG_ERG_HD inline
#endif
#ifdef __clang__
#define HMCG_ERG_UNROLL _Pragma("unroll")
#else
#define HMCG_ERG_UNROLL
#endif

namespace hmcg_host {

constexpr int erg_cols(int K) { return HMCG_ERG_COLS(K); }
// Slab sums per (window, slab): S1_c, then S2_c (both about the pivot), then the number of good draws.
constexpr int erg_items(int K) { return 2 * erg_cols(K) + 1; }
// Draw columns per window that a call reads (the host entry uploads the K diagonal columns of A as holes, never filled).
constexpr int erg_columns(int K) { return 2 * K + K * K; }
// Work area: [W][nslab_total][items] slab sums, then [W][C] pivots.
inline size_t erg_part_doubles(int W, long long nd, int K)
{
    return (size_t)W * ((size_t)pred_slabs(nd) * (size_t)erg_items(K) + (size_t)erg_cols(K));
}

// Argument rules shared by both entries; 0 or HMCG_E_BADARG with the reason in msg.  No pointer is followed.
inline int check_ergodic(const hmcg_ergodic* p, const double* mu, const double* sig2, const double* A, const double* out, const int64_t* n,
                         char* msg, size_t nmsg)
{
    if (bad_struct(p, "hmcg_ergodic", msg, nmsg) || bad_K(p->K, msg, nmsg) || bad_W(p->W, msg, nmsg) || bad_nd(p->nd, msg, nmsg) ||
        bad_nd_ld(p->nd_ld, p->nd, msg, nmsg))
        return HMCG_E_BADARG;
    if (!mu || !sig2 || !A || !out || !n) { snprintf(msg, nmsg, "mu, sig2, A, out and n are required"); return HMCG_E_BADARG; }
    return 0;
}

// One draw.  P[i + K * j] = A[i][j] (row i the from-state), already rounded where the call asks for it; the K diagonal
// slots are never read or written.  P is consumed (the elimination runs in place).  o[0..K-1] = pi, o[K..2K-1] = dur,
// o[2K] = m, o[2K + 1] = v by the rules of include/hmcg_ergodic.h: one rounded operation per step, no contraction.  Every
// index is a constant once the loops are unrolled: P, x and o stay in registers.
template <int K>
HMCG_ERG_HD void erg_draw(double* P, const double* mu, const double* sig2, double* o)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    HMCG_ERG_UNROLL
    for (int i = 0; i < K; ++i) {
        double s = P[i + K * (i == 0 ? 1 : 0)];
        HMCG_ERG_UNROLL
        for (int j = (i == 0 ? 2 : 1); j < K; ++j)
            if (j != i) s = s + P[i + K * j];
        o[K + i] = 1.0 / s;
    }
    HMCG_ERG_UNROLL
    for (int n = K - 1; n >= 1; --n) {
        double S = P[n];
        HMCG_ERG_UNROLL
        for (int j = 1; j < n; ++j) S = S + P[n + K * j];
        HMCG_ERG_UNROLL
        for (int i = 0; i < n; ++i) P[i + K * n] = P[i + K * n] / S;
        HMCG_ERG_UNROLL
        for (int i = 0; i < n; ++i) {
            HMCG_ERG_UNROLL
            for (int j = 0; j < n; ++j)
                if (i != j) {
                    const double t = P[i + K * n] * P[n + K * j];
                    P[i + K * j] = P[i + K * j] + t;
                }
        }
    }
    double x[K];
    x[0] = 1.0;
    HMCG_ERG_UNROLL
    for (int j = 1; j < K; ++j) {
        double t = x[0] * P[K * j];
        HMCG_ERG_UNROLL
        for (int i = 1; i < j; ++i) {
            const double xp = x[i] * P[i + K * j];
            t = t + xp;
        }
        x[j] = t;
    }
    double tot = x[0];
    HMCG_ERG_UNROLL
    for (int k = 1; k < K; ++k) tot = tot + x[k];
    HMCG_ERG_UNROLL
    for (int k = 0; k < K; ++k) o[k] = x[k] / tot;
    double m = o[0] * mu[0];
    HMCG_ERG_UNROLL
    for (int k = 1; k < K; ++k) {
        const double t = o[k] * mu[k];
        m = m + t;
    }
    o[2 * K] = m;
    double within = o[0] * sig2[0];
    HMCG_ERG_UNROLL
    for (int k = 1; k < K; ++k) {
        const double t = o[k] * sig2[k];
        within = within + t;
    }
    double between = 0.0;
    HMCG_ERG_UNROLL
    for (int k = 0; k < K; ++k) {
        const double e = mu[k] - m;
        const double e2 = e * e;
        const double t = o[k] * e2;
        between = k == 0 ? t : between + t;
    }
    o[2 * K + 1] = within + between;
}

}  // namespace hmcg_host
