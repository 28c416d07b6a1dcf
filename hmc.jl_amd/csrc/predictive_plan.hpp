// predictive_plan.hpp -- the argument rules of hmcg_predictive_cdf[_device] and the cut of a window's draws into slabs and
// upload chunks.  Plain C++17 without a HIP header (in the manner of plan.hpp): a g++-compiled program runs exactly the code
// the library runs, on the CPU.
//
// Slabs: draws [s * PRED_SLAB, min((s + 1) * PRED_SLAB, nd)) of every window are reduced by one block in draw order; the
// slab sums are added in slab order afterwards.  The cut depends on nd alone, so the result does not depend on how the host
// entry uploads the draws: its chunks are whole slabs (the last one ends at nd).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/hmcg.h"

namespace hmcg_host {

constexpr long long PRED_SLAB = 1024;       // draws per slab (and per block of the accumulation kernel)

inline long long pred_slabs(long long nd) { return (nd + PRED_SLAB - 1) / PRED_SLAB; }

// The largest horizon of a checked call (0: the transition draws are not read).
inline int pred_max_horizon(const hmcg_predictive& p)
{
    int m = 0;
    for (int j = 0; j < p.n_h; ++j) m = p.horizons[j] > m ? p.horizons[j] : m;
    return m;
}
// Draw columns per window that a call reads: mu, sig2, pi_end (K each) and A (K * K) with a horizon > 0.
inline int pred_columns(const hmcg_predictive& p) { return 3 * p.K + (pred_max_horizon(p) > 0 ? p.K * p.K : 0); }

// Argument rules shared by both entries; 0 or HMCG_E_BADARG with the reason in msg.  host: the grid is host memory and must be finite.
inline int check_predictive(const hmcg_predictive* p, const double* mu, const double* sig2, const double* pi_end, const double* A,
                            const double* grid, const double* cdf, bool host, char* msg, size_t nmsg)
{
    if (!p) { snprintf(msg, nmsg, "hmcg_predictive is NULL"); return HMCG_E_BADARG; }
    if (p->struct_size != (int32_t)sizeof(hmcg_predictive)) {
        snprintf(msg, nmsg, "hmcg_predictive.struct_size %d != %d", p->struct_size, (int)sizeof(hmcg_predictive));
        return HMCG_E_BADARG;
    }
    if (p->W < 1) { snprintf(msg, nmsg, "W = %d: at least one window", p->W); return HMCG_E_BADARG; }
    if (p->K < 2 || p->K > HMCG_MAXK) { snprintf(msg, nmsg, "K = %d outside 2..%d", p->K, HMCG_MAXK); return HMCG_E_BADARG; }
    if (p->G < 1 || p->G > HMCG_MAXGRID) { snprintf(msg, nmsg, "G = %d grid points outside 1..%d", p->G, HMCG_MAXGRID); return HMCG_E_BADARG; }
    if (p->n_h < 1 || p->n_h > HMCG_MAXH) { snprintf(msg, nmsg, "n_h = %d horizons outside 1..%d", p->n_h, HMCG_MAXH); return HMCG_E_BADARG; }
    for (int j = 0; j < p->n_h; ++j)
        if (p->horizons[j] < 0 || p->horizons[j] > HMCG_PRED_MAXH) {
            snprintf(msg, nmsg, "horizon %d outside 0..%d", p->horizons[j], HMCG_PRED_MAXH);
            return HMCG_E_BADARG;
        }
    if (p->nd < 1) { snprintf(msg, nmsg, "nd = %lld: at least one draw", (long long)p->nd); return HMCG_E_BADARG; }
    if (p->nd_ld < p->nd) { snprintf(msg, nmsg, "nd_ld = %lld < nd = %lld", (long long)p->nd_ld, (long long)p->nd); return HMCG_E_BADARG; }
    if (!mu || !sig2 || !pi_end || !grid || !cdf) { snprintf(msg, nmsg, "mu, sig2, pi_end, grid and cdf are required"); return HMCG_E_BADARG; }
    if (!A && pred_max_horizon(*p) > 0) { snprintf(msg, nmsg, "A is NULL with a horizon > 0"); return HMCG_E_BADARG; }
    if (host)
        for (int g = 0; g < p->G; ++g)
            if (!std::isfinite(grid[g])) { snprintf(msg, nmsg, "grid[%d] is not finite", g); return HMCG_E_BADARG; }
    return 0;
}

// Host entry: draws per upload chunk.  A chunk buffer holds W * ncol columns of that many doubles; the default keeps it near
// `target_bytes`; cap > 0 (HMCG_CHUNK_DRAWS) lowers it.  Always a whole number of slabs, at least one.
inline long long pred_chunk_draws(long long nd, int W, int ncol, long long cap, size_t target_bytes = (size_t)64 << 20)
{
    long long n = (long long)(target_bytes / (sizeof(double) * (size_t)W * (size_t)ncol));
    if (cap > 0 && cap < n) n = cap;
    n = (n + PRED_SLAB - 1) / PRED_SLAB * PRED_SLAB;          // rounded UP to whole slabs
    if (n < PRED_SLAB) n = PRED_SLAB;
    const long long all = pred_slabs(nd) * PRED_SLAB;
    return n < all ? n : all;
}

struct PredChunk { long long d0, n; };       // draws [d0, d0 + n) of every window; d0 is a slab boundary
inline std::vector<PredChunk> pred_chunks(long long nd, long long chunk_draws)
{
    std::vector<PredChunk> out;
    for (long long d0 = 0; d0 < nd; d0 += chunk_draws) out.push_back({d0, d0 + chunk_draws <= nd ? chunk_draws : nd - d0});
    return out;
}

}  // namespace hmcg_host
