// bias.hip -- uncertainty-bias moments of a window's draws, on the device.
//
// What it replaces (joe5saia/Hmc.jl): code/hassan_cdfs/bias_calcs.jl:40-53 (`calcbias`) reads `filtered_means_<date>.csv`,
// `filtered_state_probs_<date>.csv`, `filtered_trans_probs_<date>.csv` and `forecasts_<date>.csv` of every end date back from disk
// (250 000 rows each in production) and computes, over the draws i,
//   futstate[i, :] = states[i, :]' * reshape(trans[i, :], K, K)^12        = pi_end_i * A_i^h, h = 12        (:46-48)
//   covv    = cov(hcat(futstate, means))          2K x 2K, divisor n - 1, columns futstate | means           (:49)
//   nab     = mean(hcat(means, futstate), dims=1) 1 x 2K,                 columns means | futstate           (:50)
//   uncbias = nab * covv * nab'                                                                              (:51)
//   totalbias = mean(forecasts[:, 3])             forecast_error of the first horizon                        (:42)
// QUIRK, kept on purpose: nab and covv order their columns the other way round (means | futstate against futstate | means), so
// uncbias pairs the mean of mu_k with the covariance row of futstate_k.  That is what upstream computes and plots
// (thoughts/hassan_cdfs/biasestime.pdf); it is reproduced exactly.  The mean vector and the covariance matrix are written out as
// well (both in the order futstate | means), so the aligned quadratic form is one line for a caller who wants it.
//
// Shape: one block of 256 threads per (window, slab of PRED_SLAB draws); a slab is walked in tiles of 256 draws.
//   phase A  thread t takes draw t of the tile: pi_end, A, mu and the forecast-error cell are read coalesced along d (every
//            column one 2 KB line of consecutive doubles per tile), rounded as CSV cells under round5; omega = pi_end A^h by h
//            row-vector x matrix products in registers (HMCG_OMEGA_STEP of stat_device.hpp, the one expression of all three
//            features that use omega); v - p = [omega | mu | fe] - pivot goes to LDS, one row of 256 per column.
//   phase B  the items (2K (2K + 1) / 2 pair sums, 2K + 1 plain sums) are dealt round-robin to the block's four waves, so a
//            lane holds at most 39 fp64 accumulators at K = 8 instead of 153; lane l of every wave takes draws l, l + 64, l + 128,
//            l + 192 of the tile in that order: one LDS read per column (conflict-free, consecutive lanes on consecutive
//            doubles), then its wave's items from registers.
//   end      a fixed butterfly over the 64 lanes (xor 32, 16, .. 1) per item; lane 0 writes the slab sum.
// The pivot p is v of the window's draw 0.  A launch that holds draw 0 (every device-entry call; the first chunk of the host
// entry) recomputes it in every block with the same code that computes every other draw (one extra draw per block, so v - p is
// exactly 0 for a draw equal to draw 0) and the block of slab 0 files it; later chunks of the host entry read it from there.
//
// Cost: 8 (2K + K^2 + 1) bytes read per draw against K^2 h + K (2K + 1) FMAs: HBM-bound at the production shape (K = 3, h = 12:
// 128 B against 129 FMAs per draw; a CU's 4 SIMDs issue that in ~2 cycles per draw while its share of HBM delivers 128 B in ~16).
//
// Deterministic: a draw's lane and its place in that lane's sequence depend on the draw index alone; the butterfly is fixed; the
// finalize kernel adds the slab sums in slab order.  No atomics.  Numerics: fp64 throughout; NaN inputs propagate (a draw past the
// end of the slab contributes +0.0 to every sum, never a product with a NaN).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

#include "bias.hpp"
#include "stat_device.hpp"

namespace hmcg {

constexpr int BIAS_NT = 256;                 // threads per block = draws per tile
constexpr int BIAS_NW = BIAS_NT / 64;        // waves per block: the items are dealt over them
constexpr int BIAS_FIN_NT = 256;

// Columns 0..2K-1: v = [omega | mu]; column 2K: the forecast-error cell (0 when there is none).
constexpr int bias_nv(int K) { return 2 * K; }
constexpr int bias_nc(int K) { return 2 * K + 1; }
constexpr int bias_np(int K) { return K * (2 * K + 1); }
constexpr int bias_nitems(int K) { return bias_np(K) + bias_nc(K); }
// pair number of (a, b), a <= b, in the row-major upper triangle of an n x n table, and back
__host__ __device__ constexpr int bias_pair(int a, int b, int n) { return a * (2 * n - a + 1) / 2 + (b - a); }
__host__ __device__ constexpr int bias_item_a(int e, int n)
{
    if (e >= n * (n + 1) / 2) return e - n * (n + 1) / 2;       // plain sum of column a
    int a = 0;
    while (e >= n - a) { e -= n - a; ++a; }
    return a;
}
__host__ __device__ constexpr int bias_item_b(int e, int n)    // -1: a plain sum
{
    if (e >= n * (n + 1) / 2) return -1;
    int a = 0;
    while (e >= n - a) { e -= n - a; ++a; }
    return a + e;
}

struct BiasParams {
    const double* mu; const double* pi_end; const double* A; const double* fc;
    double* part;                    // [W][nslab_total][items]
    double* piv;                     // [W][2K + 1]
    long long nd, nd_ld, fc_wstride; // draws in this launch, leading dimension of the draw arrays, doubles between two windows' fc columns
    long long nslab, slab0, nslab_total;     // slabs of this launch; its first slab and the slab count of the whole run
    int horizon, round5;
};

// Item E of a draw whose columns are x[]: indices are constant expressions, so x[] and the accumulators stay in registers.
template <int K, int E>
__device__ __forceinline__ double bias_item(const double* x, double acc)
{
    constexpr int NV = bias_nv(K);
    if constexpr (E >= bias_nitems(K)) {
        return acc;
    } else {
        constexpr int a = bias_item_a(E, NV), b = bias_item_b(E, NV);
        if constexpr (b < 0) return acc + x[a];
        else return fma(x[a], x[b], acc);
    }
}
template <int K, int Q, int... I>
__device__ __forceinline__ void bias_items_of_wave(const double* x, double* acc, std::integer_sequence<int, I...>)
{
    ((acc[I] = bias_item<K, Q + BIAS_NW * I>(x, acc[I])), ...);
}

// Phase B of wave Q: items Q, Q + BIAS_NW, ... over the tile's draws lane, lane + 64, ... in that order.  From K = 6 on the four
// sub-tiles are not unrolled: their 4 (2K + 1) LDS reads in flight would cost more registers than the accumulators.
template <int K, int Q>
__device__ __forceinline__ void bias_accumulate(const double* V, int lane, double* acc)
{
    constexpr int NC = bias_nc(K), PPW = (bias_nitems(K) + BIAS_NW - 1) / BIAS_NW, UNR = K <= 5 ? BIAS_NW : 1;
#pragma unroll UNR
    for (int j = 0; j < BIAS_NW; ++j) {
        double x[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) x[c] = V[c * BIAS_NT + j * 64 + lane];
        bias_items_of_wave<K, Q>(x, acc, std::make_integer_sequence<int, PPW>{});
    }
}

template <int K>
__global__ __launch_bounds__(BIAS_NT) void bias_moments_kernel(const BiasParams p)
{
    constexpr int NV = bias_nv(K), NC = bias_nc(K), ITEMS = bias_nitems(K), PPW = (ITEMS + BIAS_NW - 1) / BIAS_NW;
    __shared__ double V[NC * BIAS_NT];                  // [column][draw of the tile]: v - p
    __shared__ double P[NC];                            // the pivot
    const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
    HMCG_STAT_SLAB(w, s, dbeg, dend, p.nslab, p.nd);
    const int ntile = (int)((dend - dbeg + BIAS_NT - 1) / BIAS_NT);
    const double* mu = p.mu + (size_t)w * K * p.nd_ld;
    const double* pie = p.pi_end + (size_t)w * K * p.nd_ld;
    const double* At = p.A ? p.A + (size_t)w * K * K * p.nd_ld : nullptr;
    const double* fc = p.fc ? p.fc + (size_t)w * (size_t)p.fc_wstride : nullptr;
    const bool own_pivot = p.slab0 == 0;                // this launch's arrays start at the window's draw 0
    if (!own_pivot) {
        if (tid < NC) P[tid] = p.piv[(size_t)w * NC + tid];
        __syncthreads();
    }
    double acc[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) acc[i] = 0.0;
    // it = -1: the pivot pass (thread 0 on draw 0), through the same code as every tile
#pragma unroll 1
    for (int it = own_pivot ? -1 : 0; it < ntile; ++it) {
        const auto [base, o, valid] = stat_tile(it, BIAS_NT, tid, dbeg, dend);
        double v[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] = 0.0;
        if (valid) {
            double wv[K];
#pragma unroll
            for (int k = 0; k < K; ++k) wv[k] = stat_in((pie + (size_t)k * p.nd_ld + base)[o], p.round5);
            if (At) {
                double a[K * K];
#pragma unroll
                for (int c = 0; c < K * K; ++c) a[c] = stat_in((At + (size_t)c * p.nd_ld + base)[o], p.round5);
#pragma unroll 1
                for (int step = 0; step < p.horizon; ++step) HMCG_OMEGA_STEP(K, wv, a, 1);
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                v[k] = wv[k];
                v[K + k] = stat_in((mu + (size_t)k * p.nd_ld + base)[o], p.round5);
            }
            if (fc) v[NV] = stat_in((fc + base)[o], p.round5);
        }
        if (it < 0) {
            if (tid == 0) {
#pragma unroll
                for (int c = 0; c < NC; ++c) P[c] = v[c];
            }
            __syncthreads();
            continue;
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) V[c * BIAS_NT + tid] = valid ? v[c] - P[c] : 0.0;
        __syncthreads();
        switch (q) {
            case 0: bias_accumulate<K, 0>(V, lane, acc); break;
            case 1: bias_accumulate<K, 1>(V, lane, acc); break;
            case 2: bias_accumulate<K, 2>(V, lane, acc); break;
            default: bias_accumulate<K, 3>(V, lane, acc); break;
        }
        __syncthreads();
    }
    if (own_pivot && s == 0 && tid < NC) p.piv[(size_t)w * NC + tid] = P[tid];
    double* row = p.part + HMCG_STAT_ROW(w, p.nslab_total, p.slab0 + s, ITEMS);
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        double t = acc[i];
        HMCG_WAVE_SUM(t);
        const int e = q + BIAS_NW * i;
        if (lane == 0 && e < ITEMS) row[e] = t;
    }
}

// One block per window: the slab sums in slab order, then mean = p + S1 / n, cov_ab = (S2_ab - S1_a S1_b / n) / (n - 1) (both
// triangles from the same expression: bit-symmetric), uncbias = nab cov nab' with nab = [mean of mu | mean of omega] against
// cov's order omega | mu (upstream's index swap, see the header comment), totalbias = p_fe + S1_fe / n.
__global__ __launch_bounds__(BIAS_FIN_NT) void bias_finalize_kernel(const double* part, const double* piv, double* out, long long nslab,
                                                                   int K, double n, int with_fc)
{
    constexpr int MAXNV = 2 * HMCG_MAXK;
    __shared__ double T[bias_nitems(HMCG_MAXK)], M[MAXNV + 1], CV[MAXNV * MAXNV], R[MAXNV];
    const int NV = 2 * K, NC = NV + 1, NP = K * (2 * K + 1), ITEMS = NP + NC;
    const int w = blockIdx.x, tid = threadIdx.x;
    for (int e = tid; e < ITEMS; e += BIAS_FIN_NT) {
        const double* col = part + (size_t)w * (size_t)nslab * (size_t)ITEMS + (size_t)e;
        HMCG_SLAB_SUM(sum, col, nslab, ITEMS);
        T[e] = sum;
    }
    __syncthreads();
    for (int c = tid; c < NC; c += BIAS_FIN_NT) M[c] = piv[(size_t)w * NC + c] + T[NP + c] / n;
    for (int e = tid; e < NV * NV; e += BIAS_FIN_NT) {
        const int i = e / NV, j = e - i * NV;
        const int a = i < j ? i : j, b = i < j ? j : i;
        const double prod = T[NP + a] * T[NP + b];
        CV[e] = (T[bias_pair(a, b, NV)] - prod / n) / (n - 1.0);
    }
    __syncthreads();
    double* o = out + (size_t)w * (size_t)HMCG_BIAS_STRIDE(K);
    for (int c = tid; c < NV; c += BIAS_FIN_NT) o[2 + c] = M[c];
    for (int e = tid; e < NV * NV; e += BIAS_FIN_NT) o[2 + NV + e] = CV[e];
    if (tid < NV) {                                     // (nab * cov)[tid], a ascending
        double r = 0.0;
        for (int a = 0; a < NV; ++a) r += M[(a + K) % NV] * CV[a * NV + tid];
        R[tid] = r;
    }
    __syncthreads();
    if (tid == 0) {
        double u = 0.0;
        for (int b = 0; b < NV; ++b) u += R[b] * M[(b + K) % NV];
        o[0] = u;
        o[1] = with_fc ? M[NV] : stat_nan();
    }
}

}  // namespace hmcg

namespace hmcg_host {

size_t bias_part_doubles(int W, long long nd, int K)
{
    return (size_t)W * ((size_t)pred_slabs(nd) * (size_t)bias_items(K) + (size_t)(2 * K + 1));
}

hipError_t launch_bias(const BiasArgs& a, hipStream_t stream)
{
    if (a.W <= 0 || a.nd <= 0) return hipSuccess;
    if (a.K < 2 || a.K > HMCG_MAXK || bias_items(a.K) != hmcg::bias_nitems(a.K)) return hipErrorInvalidValue;
    hmcg::BiasParams p{};
    p.mu = a.mu; p.pi_end = a.pi_end; p.A = a.horizon > 0 ? a.A : nullptr; p.fc = a.fc; p.fc_wstride = a.fc_wstride;
    p.part = a.part; p.piv = a.part + (size_t)a.W * (size_t)a.nslab_total * (size_t)bias_items(a.K);
    p.nd = a.nd; p.nd_ld = a.nd_ld; p.nslab = pred_slabs(a.nd); p.slab0 = a.slab0; p.nslab_total = a.nslab_total;
    p.horizon = a.horizon; p.round5 = a.round5 ? 1 : 0;
    if (a.horizon > 0 && !a.A) return hipErrorInvalidValue;
    if (!slab_range_ok(a.W, a.nd, a.nd_ld, a.slab0, a.nslab_total)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((long long)a.W * p.nslab)), block(hmcg::BIAS_NT);
#define HMCG_BIAS(K_) hipLaunchKernelGGL(hmcg::bias_moments_kernel<K_>, grid, block, 0, stream, p)
    HMCG_SWITCH_K(a.K, HMCG_BIAS)
#undef HMCG_BIAS
    return hipGetLastError();
}

hipError_t launch_bias_finalize(const double* part, double* out, int W, int K, long long nd_total, bool with_fc, hipStream_t stream)
{
    if (W <= 0) return hipSuccess;
    if (K < 2 || K > HMCG_MAXK) return hipErrorInvalidValue;
    const long long nslab = pred_slabs(nd_total);
    const double* piv = part + (size_t)W * (size_t)nslab * (size_t)bias_items(K);
    hipLaunchKernelGGL(hmcg::bias_finalize_kernel, dim3((unsigned)W), dim3(hmcg::BIAS_FIN_NT), 0, stream, part, piv, out, nslab, K,
                       (double)nd_total, with_fc ? 1 : 0);
    return hipGetLastError();
}

}  // namespace hmcg_host
