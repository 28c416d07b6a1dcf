// mixmoments_plan.hpp -- the argument rules of hmcg_mixture_moments[_device], the draw columns a call reads per window and the
// order in which its horizons are walked.  Plain C++17 without a HIP header (in the manner of predictive_plan.hpp): a
// g++-compiled program runs exactly the code the library runs, on the CPU.
//
// The cut of a window's draws into slabs and of the host entry's upload into chunks (PRED_SLAB, pred_slabs, pred_chunk_draws,
// pred_chunks) and the shared argument rules stand in stat_plan.hpp.
#pragma once
#include <cstdint>
#include <cstdio>

#include "../../include/hmcg.h"
#include "stat_plan.hpp"

namespace hmcg_host {

// Slab sums per (window, slab, horizon): P0..P4, Q1, Q2, VW, SK in that order.
constexpr int MIX_ITEMS = 9;
// Filed per (window, horizon) for the later chunks of the host entry: the pivot c and a_0, the a of the window's draw 0.
constexpr int MIX_PIVOTS = 2;

// The largest horizon and the draw columns per window of a checked call, under this feature's names (stat_plan.hpp).
inline int mix_max_horizon(const hmcg_mixmom& p) { return mixture_max_horizon(p); }
inline int mix_columns(const hmcg_mixmom& p) { return mixture_columns(p.K, mixture_max_horizon(p) > 0); }

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
    if (bad_struct(p, "hmcg_mixmom", msg, nmsg) || bad_W(p->W, msg, nmsg) || bad_K(p->K, msg, nmsg) ||
        bad_horizons(p->n_h, p->horizons, msg, nmsg) || bad_nd(p->nd, msg, nmsg) || bad_nd_ld(p->nd_ld, p->nd, msg, nmsg))
        return HMCG_E_BADARG;
    if (!mu || !sig2 || !pi_end || !out) { snprintf(msg, nmsg, "mu, sig2, pi_end and out are required"); return HMCG_E_BADARG; }
    if (!A && mix_max_horizon(*p) > 0) { snprintf(msg, nmsg, "A is NULL with a horizon > 0"); return HMCG_E_BADARG; }
    return 0;
}

}  // namespace hmcg_host
