// predictive.hip -- predictive CDFs of the regime mixture, averaged over a window's draws on the device.
//
// What it replaces (joe5saia/Hmc.jl): code/hassan_cdfs/calc_cdfs.jl reads `filtered_means_<date>.csv`, `filtered_variances_<date>.csv`
// and `filtered_state_probs_<date>.csv` of every end date back from disk (250 000 rows each in production) and evaluates, for
// every draw i and every grid point y of -5:.25:15,
//   F_i(y) = sum_k pi_i[k] * Phi((y - mu_i[k]) / sqrt(sig2_i[k]))                                        (:39)
// then averages over the draws (`expectationsbar`, :41).  Here the draws are read where they lie in HBM.  Horizons h > 0 use
// the weights pi_i * A_i^h, the state law of forecast (src/Hmc.jl:662-663): the h-step-ahead predictive distribution.
//
// Shape: one block per (window, slab of PRED_SLAB draws, 128 (horizon, grid point) items).  A tile of 64 draws is staged in LDS --
// per draw and state mu_k and c_k = 1 / (sqrt 2 * sqrt(sig2_k)) side by side, and the n_h * K weights, built per (draw, horizon) by
// h successive row-vector x matrix products over the tile's transition draws (the tile and its walk: mixture_tile.hpp).  Each thread then
// owns one (horizon, grid point) and walks the tile in draw order: every lane reads the same mu, c (one broadcast ds_read_b128),
// Phi = erfc(-(y - mu) c) / 2.  fp64 VALU work by construction: 8 (3K [+ K^2]) bytes read per draw against K * n_h * G erfc.
//
// Numerics: with round5 every input is rounded as a CSV cell is (round5.hpp).  No special cases: a zero variance gives c = inf,
// so Phi is 0 or 1 and NaN where y == mu; a NaN term times a zero weight stays NaN.  Deterministic: a thread adds its slab's draws
// in draw order and writes the slab sum; predictive_finalize_kernel adds the slab sums in slab order and divides by nd.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "predictive.hpp"
#include "mixture_tile.hpp"

namespace hmcg {

constexpr int PRED_FIN_NT = 256;

struct PredictiveParams {
    const double* mu; const double* sig2; const double* pi_end; const double* A; const double* grid;
    double* part;                    // [W][nslab_total][items]
    long long nd, nd_ld;             // draws in this launch, leading dimension of the draw arrays
    long long nslab, slab0, nslab_total;     // slabs of this launch; its first slab and the slab count of the whole run
    int G, n_h, items, round5;
    int hz[HMCG_MAXH];
};

template <int K>
__global__ __launch_bounds__(MIXTILE_NT) void predictive_cdf_kernel(const PredictiveParams p)
{
    extern __shared__ double pred_lds[];
    const int n_h = p.n_h;
    HMCG_MIX_TILE_LDS(K, pred_lds, n_h, MC, Ws, As);
    const int tid = threadIdx.x;
    HMCG_STAT_SLAB(w, s, dbeg, dend, p.nslab, p.nd);
    const int e = (int)blockIdx.y * MIXTILE_NT + tid;    // this thread's item: horizon j, grid point g
    const bool live = e < p.items;
    const int j = live ? e / p.G : 0, g = live ? e - j * p.G : 0;
    const double y = stat_in(p.grid[g], p.round5);
    const double* mu = p.mu + (size_t)w * K * p.nd_ld;
    const double* sig2 = p.sig2 + (size_t)w * K * p.nd_ld;
    const double* pie = p.pi_end + (size_t)w * K * p.nd_ld;
    const double* At = p.A ? p.A + (size_t)w * K * K * p.nd_ld : nullptr;
    double acc = 0.0;
#define PRED_DRAW(dd) (size_t)(d0 + (dd))
    for (long long d0 = dbeg; d0 < dend; d0 += MIXTILE_TD) {
        const int nv = dend - d0 < MIXTILE_TD ? (int)(dend - d0) : MIXTILE_TD;
        HMCG_MIX_TILE_STAGE(K, MC, Ws, As, mu, sig2, pie, At, p, PRED_DRAW, nv, n_h, tid);
        if (live) HMCG_MIX_TILE_WALK(K, MC, Ws, nv, n_h, j, y, acc);
        __syncthreads();
    }
#undef PRED_DRAW
    if (live) p.part[HMCG_STAT_ROW(w, p.nslab_total, p.slab0 + s, p.items) + (size_t)e] = acc;
}

__global__ __launch_bounds__(PRED_FIN_NT) void predictive_finalize_kernel(const double* part, double* cdf, long long nslab, int items,
                                                                         long long total, double nd)
{
    const long long idx = (long long)blockIdx.x * PRED_FIN_NT + threadIdx.x;
    if (idx >= total) return;
    const long long w = idx / items;
    const int e = (int)(idx - w * items);
    const double* col = part + (size_t)w * (size_t)nslab * (size_t)items + (size_t)e;
    HMCG_SLAB_SUM(sum, col, nslab, items);
    cdf[idx] = sum / nd;
}

}  // namespace hmcg

namespace hmcg_host {

size_t predictive_part_doubles(int W, long long nd, int n_h, int G) { return (size_t)W * (size_t)pred_slabs(nd) * (size_t)n_h * (size_t)G; }

hipError_t launch_predictive(const PredictiveArgs& a, hipStream_t stream)
{
    if (a.W <= 0 || a.nd <= 0) return hipSuccess;
    hmcg::PredictiveParams p{};
    p.mu = a.mu; p.sig2 = a.sig2; p.pi_end = a.pi_end; p.A = a.A; p.grid = a.grid; p.part = a.part;
    p.nd = a.nd; p.nd_ld = a.nd_ld; p.nslab = pred_slabs(a.nd); p.slab0 = a.slab0; p.nslab_total = a.nslab_total;
    p.G = a.G; p.n_h = a.n_h; p.items = a.n_h * a.G; p.round5 = a.round5 ? 1 : 0;
    const bool with_A = fill_horizons(a.n_h, a.horizons, p.hz);
    if (with_A && !a.A) return hipErrorInvalidValue;
    if (!with_A) p.A = nullptr;
    // nd_ld >= nd is part of the rule; check_predictive has enforced it ahead of every launch already
    if (!slab_range_ok(a.W, a.nd, a.nd_ld, a.slab0, a.nslab_total)) return hipErrorInvalidValue;
    const size_t lds = mixture_lds_bytes(a.K, a.n_h, with_A);
    const dim3 grid((unsigned)((long long)a.W * p.nslab), (unsigned)((p.items + hmcg::MIXTILE_NT - 1) / hmcg::MIXTILE_NT)), block(hmcg::MIXTILE_NT);
#define HMCG_PRED(K_) HMCG_LAUNCH_LDS(hmcg::predictive_cdf_kernel<K_>, grid, block, lds, stream, p)
    HMCG_SWITCH_K(a.K, HMCG_PRED)
#undef HMCG_PRED
    return hipGetLastError();
}

hipError_t launch_predictive_finalize(const double* part, double* cdf, int W, int n_h, int G, long long nd_total, hipStream_t stream)
{
    const long long total = (long long)W * n_h * G;
    if (total <= 0) return hipSuccess;
    const unsigned nb = (unsigned)((total + hmcg::PRED_FIN_NT - 1) / hmcg::PRED_FIN_NT);
    hipLaunchKernelGGL(hmcg::predictive_finalize_kernel, dim3(nb), dim3(hmcg::PRED_FIN_NT), 0, stream, part, cdf, pred_slabs(nd_total),
                       n_h * G, total, (double)nd_total);
    return hipGetLastError();
}

}  // namespace hmcg_host
