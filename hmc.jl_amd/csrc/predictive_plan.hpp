// predictive_plan.hpp -- the argument rules of hmcg_predictive_cdf[_device] and the draw columns a call reads per window.
// Plain C++17 without a HIP header (in the manner of plan.hpp): a g++-compiled program runs exactly the code the library runs,
// on the CPU.  The cut of a window's draws into slabs and upload chunks and the shared argument rules stand in stat_plan.hpp.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/hmcg.h"
#include "stat_plan.hpp"

namespace hmcg_host {

// The largest horizon and the draw columns per window of a checked call, under this feature's names (stat_plan.hpp).
inline int pred_max_horizon(const hmcg_predictive& p) { return mixture_max_horizon(p); }
inline int pred_columns(const hmcg_predictive& p) { return mixture_columns(p.K, mixture_max_horizon(p) > 0); }

// Argument rules shared by both entries; 0 or HMCG_E_BADARG with the reason in msg.  host: the grid is host memory and must be finite.
inline int check_predictive(const hmcg_predictive* p, const double* mu, const double* sig2, const double* pi_end, const double* A,
                            const double* grid, const double* cdf, bool host, char* msg, size_t nmsg)
{
    if (bad_struct(p, "hmcg_predictive", msg, nmsg) || bad_W(p->W, msg, nmsg) || bad_K(p->K, msg, nmsg)) return HMCG_E_BADARG;
    if (p->G < 1 || p->G > HMCG_MAXGRID) { snprintf(msg, nmsg, "G = %d grid points outside 1..%d", p->G, HMCG_MAXGRID); return HMCG_E_BADARG; }
    if (bad_horizons(p->n_h, p->horizons, msg, nmsg) || bad_nd(p->nd, msg, nmsg) || bad_nd_ld(p->nd_ld, p->nd, msg, nmsg)) return HMCG_E_BADARG;
    if (!mu || !sig2 || !pi_end || !grid || !cdf) { snprintf(msg, nmsg, "mu, sig2, pi_end, grid and cdf are required"); return HMCG_E_BADARG; }
    if (!A && pred_max_horizon(*p) > 0) { snprintf(msg, nmsg, "A is NULL with a horizon > 0"); return HMCG_E_BADARG; }
    if (host)
        for (int g = 0; g < p->G; ++g)
            if (!std::isfinite(grid[g])) { snprintf(msg, nmsg, "grid[%d] is not finite", g); return HMCG_E_BADARG; }
    return 0;
}

}  // namespace hmcg_host
