// ergodic.hip -- the ergodic regime law, expected durations and long-run moments of a window's draws, on the device.
//
// Every other draw statistic weights the regimes by omega = pi_end A^h at a fixed horizon; this is the limit h -> infinity, the
// numbers a regime-switching paper reports first: per draw the stationary law pi of the transition matrix (by the
// subtraction-free GTH elimination, erg_draw of ergodic_plan.hpp -- why not a linear solve is said there), the expected
// duration of each regime, and the mean and variance of the series the draw implies in the long run.  The per-draw columns
// can be kept (the layout of the chain entries, which then give their quantiles, densities and autocorrelations); per window
// the mean and variance over the good draws (all columns finite) are reduced here.  The rules stand in include/hmcg_ergodic.h.
//
// Shape: one block of 256 threads per (window, slab of PRED_SLAB draws); a slab is walked in tiles of 256 draws.  Thread t takes
// draw t of the tile: the K^2 - K off-diagonal columns of A (the diagonal is never read), mu and sig2 are read coalesced along
// d (every column one 2 KB line of consecutive doubles per tile, a scalar base and a 32-bit lane offset), all of them before
// the first is rounded as a CSV cell under round5.  P stays in registers, the loops of erg_draw unrolled to constant indices.
// Each thread adds x - p and (x - p)^2 of its good draws to its own 2 C accumulators and counts them; at the end of the slab a
// fixed butterfly over the 64 lanes (xor 32, 16, .. 1) and then the four waves in wave order.
// The pivot p is the column vector of the window's draw 0 when that draw is good, zeros otherwise.  A launch that holds draw 0
// (every device-entry call; the first chunk of the host entry) computes it in every block through the code every other draw
// goes through (pass -1) and the block of slab 0 files it; later chunks of the host entry read it from there.
//
// Cost: 8 (K^2 + K) bytes read and, with cols, 8 (2K + 2) written per draw against ~K^3 / 3 multiply-adds and 2K + K (K - 1) / 2
// divisions: HBM-bound at K = 3 (96 B per draw); at K = 8 the 44 fp64 divisions per draw weigh beside the 576 B.
//
// Deterministic: a draw's thread and its place in that thread's sequence depend on the draw index alone; the butterfly and the
// wave order are fixed; the finalize kernel adds the slab sums in slab order.  No atomics.  Numerics: fp64 throughout.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ergodic.hpp"
#include "stat_device.hpp"

namespace hmcg {

constexpr int ERG_NT = 256;                  // threads per block = draws per tile
constexpr int ERG_NW = ERG_NT / 64;
constexpr int ERG_FIN_NT = 64;

struct ErgParams {
    const double* mu; const double* sig2; const double* A;
    double* cols;                    // [W][C][nd_ld] or NULL
    double* part;                    // [W][nslab_total][items]
    double* piv;                     // [W][C]
    long long nd, nd_ld;             // draws in this launch, leading dimension of the draw arrays and of cols
    long long nslab, slab0, nslab_total;     // slabs of this launch; its first slab and the slab count of the whole run
    int round5;
};

template <int K>
__global__ __launch_bounds__(ERG_NT) void ergodic_kernel(const ErgParams p)
{
    constexpr int C = hmcg_host::erg_cols(K), ITEMS = hmcg_host::erg_items(K);
    __shared__ double Pv[C];                            // the pivot
    __shared__ double R[ERG_NW][ITEMS];
    const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
    HMCG_STAT_SLAB(w, s, dbeg, dend, p.nslab, p.nd);
    const int ntile = (int)((dend - dbeg + ERG_NT - 1) / ERG_NT);
    const double* mu = p.mu + (size_t)w * K * p.nd_ld;
    const double* sg = p.sig2 + (size_t)w * K * p.nd_ld;
    const double* At = p.A + (size_t)w * K * K * p.nd_ld;
    double* cl = p.cols ? p.cols + (size_t)w * C * p.nd_ld : nullptr;
    double* piv = p.piv + (size_t)w * C;
    const bool own_pivot = p.slab0 == 0;                // this launch's arrays start at the window's draw 0
    if (!own_pivot) {
        if (tid < C) Pv[tid] = piv[tid];
        __syncthreads();
    }
    double s1[C], s2[C], ng = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) s1[c] = s2[c] = 0.0;
    // it = -1: the pivot pass (thread 0 on draw 0), through the same code as every tile
#pragma unroll 1
    for (int it = own_pivot ? -1 : 0; it < ntile; ++it) {
        const auto [base, o, valid] = stat_tile(it, ERG_NT, tid, dbeg, dend);
        if (valid) {
            // every column is loaded before any is rounded: a rounding between two loads would make the second wait for the first
            double a[K * K], m[K], v[K], x[C];
#pragma unroll
            for (int j = 0; j < K; ++j)
#pragma unroll
                for (int i = 0; i < K; ++i)
                    if (i != j) a[i + K * j] = (At + (size_t)(i + K * j) * p.nd_ld + base)[o];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                m[k] = (mu + (size_t)k * p.nd_ld + base)[o];
                v[k] = (sg + (size_t)k * p.nd_ld + base)[o];
            }
            if (p.round5) {                                      // stat_in of stat_device.hpp, taken once for all cells
#pragma unroll
                for (int j = 0; j < K; ++j)
#pragma unroll
                    for (int i = 0; i < K; ++i)
                        if (i != j) a[i + K * j] = round5(a[i + K * j]);
#pragma unroll
                for (int k = 0; k < K; ++k) { m[k] = round5(m[k]); v[k] = round5(v[k]); }
            }
            hmcg_host::erg_draw<K>(a, m, v, x);
            bool good = true;
#pragma unroll
            for (int c = 0; c < C; ++c) good = good && isfinite(x[c]);
            if (it < 0) {
#pragma unroll
                for (int c = 0; c < C; ++c) Pv[c] = good ? x[c] : 0.0;
            } else {
                if (cl) {
#pragma unroll
                    for (int c = 0; c < C; ++c) (cl + (size_t)c * p.nd_ld + base)[o] = x[c];
                }
                if (good) {
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const double d = x[c] - Pv[c];
                        s1[c] += d;
                        s2[c] = fma(d, d, s2[c]);
                    }
                    ng += 1.0;
                }
            }
        }
        if (it < 0) __syncthreads();
    }
    if (own_pivot && s == 0 && tid < C) piv[tid] = Pv[tid];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        double t = s1[c], u = s2[c];
        HMCG_WAVE_SUM(t);
        HMCG_WAVE_SUM(u);
        if (lane == 0) { R[q][c] = t; R[q][C + c] = u; }
    }
    HMCG_WAVE_SUM(ng);
    if (lane == 0) R[q][2 * C] = ng;
    __syncthreads();
    if (tid < ITEMS) {
        double t = R[0][tid];
#pragma unroll
        for (int x = 1; x < ERG_NW; ++x) t += R[x][tid];
        double* row = p.part + HMCG_STAT_ROW(w, p.nslab_total, p.slab0 + s, ITEMS);
        row[tid] = t;
    }
}

// One block per window: the slab sums in slab order, then mean = p + S1 / g, variance = (S2 - S1 S1 / g) / (g - 1) per column
// over the g good draws, and the two counts.
__global__ __launch_bounds__(ERG_FIN_NT) void ergodic_finalize_kernel(const double* part, const double* piv, double* out, long long* n,
                                                                    long long nslab, int K, long long nd)
{
#pragma clang fp contract(off)
    __shared__ double T[hmcg_host::erg_items(HMCG_MAXK)];
    const int C = hmcg_host::erg_cols(K), ITEMS = hmcg_host::erg_items(K);
    const int w = blockIdx.x, tid = threadIdx.x;
    if (tid < ITEMS) {
        const double* col = part + (size_t)w * (size_t)nslab * (size_t)ITEMS + (size_t)tid;
        HMCG_SLAB_SUM(sum, col, nslab, ITEMS);
        T[tid] = sum;
    }
    __syncthreads();
    const double g = T[2 * C];
    if (tid < C) {
        const double S1 = T[tid], S2 = T[C + tid];
        double* o = out + ((size_t)w * (size_t)C + (size_t)tid) * 2;
        o[0] = piv[(size_t)w * C + tid] + S1 / g;
        o[1] = (S2 - S1 * S1 / g) / (g - 1.0);
    }
    if (tid == 0) {
        const long long good = (long long)g;
        n[(size_t)w * 2] = good;
        n[(size_t)w * 2 + 1] = nd - good;
    }
}

}  // namespace hmcg

namespace hmcg_host {

hipError_t launch_ergodic(const ErgArgs& a, hipStream_t stream)
{
    if (a.W <= 0 || a.nd <= 0) return hipSuccess;
    if (a.K < 2 || a.K > HMCG_MAXK || !a.mu || !a.sig2 || !a.A || !a.part) return hipErrorInvalidValue;
    hmcg::ErgParams p{};
    p.mu = a.mu; p.sig2 = a.sig2; p.A = a.A; p.cols = a.cols;
    p.part = a.part; p.piv = a.part + (size_t)a.W * (size_t)a.nslab_total * (size_t)erg_items(a.K);
    p.nd = a.nd; p.nd_ld = a.nd_ld; p.nslab = pred_slabs(a.nd); p.slab0 = a.slab0; p.nslab_total = a.nslab_total;
    p.round5 = a.round5 ? 1 : 0;
    if (!slab_range_ok(a.W, a.nd, a.nd_ld, a.slab0, a.nslab_total)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((long long)a.W * p.nslab)), block(hmcg::ERG_NT);
#define HMCG_ERG(K_) hipLaunchKernelGGL(hmcg::ergodic_kernel<K_>, grid, block, 0, stream, p)
    HMCG_SWITCH_K(a.K, HMCG_ERG)
#undef HMCG_ERG
    return hipGetLastError();
}

hipError_t launch_ergodic_finalize(const double* part, double* out, long long* n, int W, int K, long long nd_total, hipStream_t stream)
{
    if (W <= 0) return hipSuccess;
    if (K < 2 || K > HMCG_MAXK) return hipErrorInvalidValue;
    const long long nslab = pred_slabs(nd_total);
    const double* piv = part + (size_t)W * (size_t)nslab * (size_t)erg_items(K);
    hipLaunchKernelGGL(hmcg::ergodic_finalize_kernel, dim3((unsigned)W), dim3(hmcg::ERG_FIN_NT), 0, stream, part, piv, out, n, nslab, K,
                       nd_total);
    return hipGetLastError();
}

}  // namespace hmcg_host
