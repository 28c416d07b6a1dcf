// mixmoments_plan.hpp -- the argument rules of hmcg_mixture_moments[_device], the draw columns a call reads per window and the
// order in which its horizons are walked.  Plain C++17 without a HIP header (in the manner of predictive_plan.hpp): a
// g++-compiled program runs exactly the code the library runs, on the CPU.
//
// The cut of a window's draws into slabs and of the host entry's upload into chunks is the one of the predictive CDFs
// (PRED_SLAB, pred_slabs, pred_chunk_draws, pred_chunks of predictive_plan.hpp): draws [s * PRED_SLAB, min((s + 1) * PRED_SLAB, nd))
// are reduced by one block, the slab sums are added in slab order afterwards, and an upload chunk is a whole number of slabs.
#pragma once
#include <cstdint>
#include <cstdio>

#include "../../include/hmcg.h"
#include "predictive_plan.hpp"

namespace hmcg_host {

// Slab sums per (window, slab, horizon): P0..P4, Q1, Q2, VW, SK in that order.
constexpr int MIX_ITEMS = 9;
// Filed per (window, horizon) for the later chunks of the host entry: the pivot c and a_0, the a of the window's draw 0.
constexpr int MIX_PIVOTS = 2;

inline int mix_max_horizon(const hmcg_mixmom& p)
{
    int m = 0;
    for (int j = 0; j < p.n_h; ++j) m = p.horizons[j] > m ? p.horizons[j] : m;
    return m;
}
// Draw columns per window that a call reads: mu, sig2, pi_end (K each) and A (K * K) with a horizon > 0.
inline int mix_columns(const hmcg_mixmom& p) { return 3 * p.K + (mix_max_horizon(p) > 0 ? p.K * p.K : 0); }

// The ascending walk: omega is carried along one chain of mix_max_horizon products, and at position i of the walk the chain
// stands at hz[i] = horizons[slot[i]] (hz ascending; equal horizons keep their order).  Every horizon gets the bits it would get
// alone, for the cost of h_max steps instead of the sum.  Entries from n_h on are zero.
struct MixWalk { int hz[HMCG_MAXH]; int slot[HMCG_MAXH]; };
inline MixWalk mix_walk(const hmcg_mixmom& p)
{
    MixWalk w{};
    for (int j = 0; j < p.n_h; ++j) {                     // insertion sort, stable
        int i = j;
        for (; i > 0 && w.hz[i - 1] > p.horizons[j]; --i) { w.hz[i] = w.hz[i - 1]; w.slot[i] = w.slot[i - 1]; }
        w.hz[i] = p.horizons[j];
        w.slot[i] = j;
    }
    return w;
}

// Argument rules shared by both entries; 0 or HMCG_E_BADARG with the reason in msg.  No pointer is followed.
inline int check_mixmom(const hmcg_mixmom* p, const double* mu, const double* sig2, const double* pi_end, const double* A,
                        const double* out, char* msg, size_t nmsg)
{
    if (!p) { snprintf(msg, nmsg, "hmcg_mixmom is NULL"); return HMCG_E_BADARG; }
    if (p->struct_size != (int32_t)sizeof(hmcg_mixmom)) {
        snprintf(msg, nmsg, "hmcg_mixmom.struct_size %d != %d", p->struct_size, (int)sizeof(hmcg_mixmom));
        return HMCG_E_BADARG;
    }
    if (p->W < 1) { snprintf(msg, nmsg, "W = %d: at least one window", p->W); return HMCG_E_BADARG; }
    if (p->K < 2 || p->K > HMCG_MAXK) { snprintf(msg, nmsg, "K = %d outside 2..%d", p->K, HMCG_MAXK); return HMCG_E_BADARG; }
    if (p->n_h < 1 || p->n_h > HMCG_MAXH) { snprintf(msg, nmsg, "n_h = %d horizons outside 1..%d", p->n_h, HMCG_MAXH); return HMCG_E_BADARG; }
    for (int j = 0; j < p->n_h; ++j)
        if (p->horizons[j] < 0 || p->horizons[j] > HMCG_PRED_MAXH) {
            snprintf(msg, nmsg, "horizon %d outside 0..%d", p->horizons[j], HMCG_PRED_MAXH);
            return HMCG_E_BADARG;
        }
    if (p->nd < 1) { snprintf(msg, nmsg, "nd = %lld: at least one draw", (long long)p->nd); return HMCG_E_BADARG; }
    if (p->nd_ld < p->nd) { snprintf(msg, nmsg, "nd_ld = %lld < nd = %lld", (long long)p->nd_ld, (long long)p->nd); return HMCG_E_BADARG; }
    if (!mu || !sig2 || !pi_end || !out) { snprintf(msg, nmsg, "mu, sig2, pi_end and out are required"); return HMCG_E_BADARG; }
    if (!A && mix_max_horizon(*p) > 0) { snprintf(msg, nmsg, "A is NULL with a horizon > 0"); return HMCG_E_BADARG; }
    return 0;
}

}  // namespace hmcg_host
