// autocorr_plan.hpp -- the argument rules of hmcg_chain_autocorr[_device] and the split of a block's 256 threads over lags and
// draws.  Plain C++17 without a HIP header (in the manner of density_plan.hpp): a g++-compiled program runs exactly the code the
// library runs, on the CPU; the kernels call acf_plan too.
//
// A block owns one (window, column) and walks the 1024-draw slabs of a launch in order.  A thread holds ACF_J adjacent lags
// l0 .. l0 + ACF_J - 1, l0 = ACF_J * (thread % lag_threads), and the draws [group * group_draws, (group + 1) * group_draws) of
// the slab, group = thread / lag_threads: lag_threads is the smallest power of two >= 2 that covers L + 1 lags, so with a short
// lag window the slab's draws are shared among more groups.  The groups' sums of a lag are added in group order.  The split
// depends on L alone.
#pragma once
#include <cstdint>
#include <cstdio>

#include "../../include/hmcg.h"
#include "stat_plan.hpp"

#ifdef __HIPCC__
#define HMCG_ACF_HD __host__ __device__ __forceinline__
#else
#define HMCG_ACF_HD inline
#endif

namespace hmcg_host {

constexpr int ACF_NT = 256;                  // threads per block
constexpr int ACF_J = 8;                     // adjacent lags per thread = draws per register tile
constexpr int ACF_SUMS = 6;                  // S1, S2 of [0, h), [h, n - h), [n - h, n)
static_assert(PRED_SLAB % ACF_NT == 0 && PRED_SLAB % ACF_J == 0, "a slab is a whole number of tiles");
static_assert(HMCG_ACF_MAXLAG <= PRED_SLAB, "the halo of a slab is at most one slab");

struct AcfPlan {
    int lags_r;         // L + 1 rounded up to ACF_J: the lags computed, and the halo of a slab in draws
    int lag_threads;    // threads that share the lags, a power of two in 2..ACF_NT
    int groups;         // ACF_NT / lag_threads
    int group_draws;    // PRED_SLAB / groups, a multiple of ACF_J
};

HMCG_ACF_HD AcfPlan acf_plan(int L)
{
    AcfPlan p;
    p.lags_r = (L + ACF_J) / ACF_J * ACF_J;
    p.lag_threads = 2;
    while (p.lag_threads * ACF_J < L + 1) p.lag_threads *= 2;
    p.groups = ACF_NT / p.lag_threads;
    p.group_draws = (int)(PRED_SLAB / p.groups);
    return p;
}

// Doubles of the work area per (window, column): L + 1 running lag sums, ACF_SUMS running sums, the pivot, 2 L edge values.
HMCG_ACF_HD long long acf_work_doubles(int L) { return (long long)(L + 1) + ACF_SUMS + 1 + 2LL * L; }

// Draws in front of an upload chunk that starts at draw d0.
HMCG_ACF_HD long long acf_pre(long long d0, int L) { return d0 < (long long)L ? d0 : (long long)L; }

// Argument rules shared by both entries; 0 or HMCG_E_BADARG with the reason in msg.  No pointer is followed.
inline int check_autocorr(const hmcg_autocorr* p, const double* x, const double* acov, const double* diag, char* msg, size_t nmsg)
{
    // n and n - l are fp64 factors
    if (bad_struct(p, "hmcg_autocorr", msg, nmsg) || bad_W(p->W, msg, nmsg) || bad_C(p->C, msg, nmsg) || bad_nd(p->nd, msg, nmsg) ||
        bad_exact_nd(p->nd, msg, nmsg) || bad_nd_ld(p->nd_ld, p->nd, msg, nmsg))
        return HMCG_E_BADARG;
    if (p->L < 0 || p->L > HMCG_ACF_MAXLAG) { snprintf(msg, nmsg, "L = %d lags outside 0..%d", p->L, HMCG_ACF_MAXLAG); return HMCG_E_BADARG; }
    if ((long long)p->L > p->nd - 1) { snprintf(msg, nmsg, "L = %d exceeds nd - 1 = %lld", p->L, (long long)p->nd - 1); return HMCG_E_BADARG; }
    if (bad_WC(p->W, p->C, msg, nmsg)) return HMCG_E_BADARG;        // both kernels
    if (!x || !acov || !diag) { snprintf(msg, nmsg, "x, acov and diag are required"); return HMCG_E_BADARG; }
    return 0;
}

}  // namespace hmcg_host
