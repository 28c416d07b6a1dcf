// bias_plan.hpp -- the argument rules of hmcg_bias_moments[_device] and the draw columns a call reads per window.  Plain
// C++17 without a HIP header (in the manner of predictive_plan.hpp): a g++-compiled program runs exactly the code the library
// runs, on the CPU.
//
// The cut of a window's draws into slabs and of the host entry's upload into chunks (PRED_SLAB, pred_slabs, pred_chunk_draws,
// pred_chunks) and the shared argument rules stand in stat_plan.hpp.
#pragma once
#include <cstdint>
#include <cstdio>

#include "../../include/hmcg.h"
#include "stat_plan.hpp"

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
    if (bad_struct(p, "hmcg_bias", msg, nmsg) || bad_W(p->W, msg, nmsg) || bad_K(p->K, msg, nmsg) || bad_horizon(p->horizon, msg, nmsg) ||
        bad_nd(p->nd, msg, nmsg) || bad_nd_ld(p->nd_ld, p->nd, msg, nmsg))
        return HMCG_E_BADARG;
    if (!mu || !pi_end || !out) { snprintf(msg, nmsg, "mu, pi_end and out are required"); return HMCG_E_BADARG; }
    if (!A && p->horizon > 0) { snprintf(msg, nmsg, "A is NULL with horizon > 0"); return HMCG_E_BADARG; }
    if (fcast && (p->H < 1 || p->H > HMCG_MAXH)) { snprintf(msg, nmsg, "fcast given with H = %d outside 1..%d", p->H, HMCG_MAXH); return HMCG_E_BADARG; }
    return 0;
}

}  // namespace hmcg_host
