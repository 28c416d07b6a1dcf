// bias_plan.hpp -- the argument rules of hmcg_bias_moments[_device] and the draw columns a call reads per window.  Plain
// C++17 without a HIP header (in the manner of predictive_plan.hpp): a g++-compiled program runs exactly the code the library
// runs, on the CPU.
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

// Columns of the moment block: v = [futstate | means].
inline int bias_vars(int K) { return 2 * K; }
// Slab sums per (window, slab): the pair sums S2_ab (a <= b, row-major upper triangle), then S1_a, then the sum of the
// forecast-error column.
inline int bias_items(int K) { return bias_vars(K) * (bias_vars(K) + 1) / 2 + bias_vars(K) + 1; }

// Draw columns per window that a call reads: mu and pi_end (K each), A (K * K) with horizon > 0, one forecast-error column
// when fcast is given.
inline int bias_columns(const hmcg_bias& p, bool with_fcast) { return 2 * p.K + (p.horizon > 0 ? p.K * p.K : 0) + (with_fcast ? 1 : 0); }

// Argument rules shared by both entries; 0 or HMCG_E_BADARG with the reason in msg.  No pointer is followed.
inline int check_bias(const hmcg_bias* p, const double* mu, const double* pi_end, const double* A, const double* fcast, const double* out,
                      char* msg, size_t nmsg)
{
    if (!p) { snprintf(msg, nmsg, "hmcg_bias is NULL"); return HMCG_E_BADARG; }
    if (p->struct_size != (int32_t)sizeof(hmcg_bias)) {
        snprintf(msg, nmsg, "hmcg_bias.struct_size %d != %d", p->struct_size, (int)sizeof(hmcg_bias));
        return HMCG_E_BADARG;
    }
    if (p->W < 1) { snprintf(msg, nmsg, "W = %d: at least one window", p->W); return HMCG_E_BADARG; }
    if (p->K < 2 || p->K > HMCG_MAXK) { snprintf(msg, nmsg, "K = %d outside 2..%d", p->K, HMCG_MAXK); return HMCG_E_BADARG; }
    if (p->horizon < 0 || p->horizon > HMCG_PRED_MAXH) {
        snprintf(msg, nmsg, "horizon %d outside 0..%d", p->horizon, HMCG_PRED_MAXH);
        return HMCG_E_BADARG;
    }
    if (p->nd < 1) { snprintf(msg, nmsg, "nd = %lld: at least one draw", (long long)p->nd); return HMCG_E_BADARG; }
    if (p->nd_ld < p->nd) { snprintf(msg, nmsg, "nd_ld = %lld < nd = %lld", (long long)p->nd_ld, (long long)p->nd); return HMCG_E_BADARG; }
    if (!mu || !pi_end || !out) { snprintf(msg, nmsg, "mu, pi_end and out are required"); return HMCG_E_BADARG; }
    if (!A && p->horizon > 0) { snprintf(msg, nmsg, "A is NULL with horizon > 0"); return HMCG_E_BADARG; }
    if (fcast && (p->H < 1 || p->H > HMCG_MAXH)) { snprintf(msg, nmsg, "fcast given with H = %d outside 1..%d", p->H, HMCG_MAXH); return HMCG_E_BADARG; }
    return 0;
}

}  // namespace hmcg_host
