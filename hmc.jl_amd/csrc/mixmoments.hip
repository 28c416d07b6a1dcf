// mixmoments.hip -- moments of the predictive regime mixture of a window's draws, on the device.
//
// What it replaces (joe5saia/Hmc.jl): code/skewness.jl:31-43 builds the end date's inflation law, the K-component normal mixture
// sum_k p_k N(mu_k, sig2_k), from one row of the three posterior-summary files and draws 10 000 000 variates from it to estimate
// one standardised third moment; code/alt_forecasts.jl:30-35 sets the plug-in mean dot(pi' * A^12, mu) of the summary rows
// beside the draw mean of forecast_12.  Both ask about the predictive law y_{T+h} ~ sum_k omega_k N(mu_k, sig2_k),
// omega = pi_end A^h, and put posterior means where the draws belong.  With the draws at hand the exact answer is a sum over
// draws: the posterior predictive law is the mixture of all nd * K components, so its raw moments about any point c are draw
// sums of the per-draw closed forms (X ~ N(delta, v): E X = delta, E X^2 = delta^2 + v, E X^3 = delta (delta^2 + 3 v),
// E X^4 = delta^4 + 6 delta^2 v + 3 v^2).  Beside the pooled mean, variance, skewness and excess kurtosis the kernel sums what
// a plug-in hides: the per-draw variance and skewness (normalised by s_d = sum_k omega_k as skewness.jl:33 normalises p) and
// the first two moments over the draws of the per-draw mean.  The formulas stand in include/hmcg.h.
//
// Shape: one block of 256 threads per (window, slab of PRED_SLAB draws); a slab is walked in tiles of 256 draws.  Thread t takes
// draw t of the tile: pi_end, A, mu and sig2 are read coalesced along d (every column one 2 KB line of consecutive doubles per
// tile, a scalar base and a 32-bit lane offset), rounded as CSV cells under round5.  A stays in registers; omega = pi_end A^h
// by row-vector x matrix products (HMCG_OMEGA_STEP of stat_device.hpp, the one expression of all three features that use
// omega).  The horizons are walked in ascending order along one chain (mix_walk): h_max
// products instead of the sum, the same bits for every horizon, equal bits for equal horizons.  At every stop of the walk the
// thread adds the draw's nine terms to its own nine accumulators of that stop; the accumulators are indexed by unrolled,
// constant stop numbers and stay in registers (the kernel is built for up to 2 and for up to HMCG_MAXH stops).  At the end
// of the slab a fixed butterfly over the 64 lanes (xor 32, 16, .. 1) and then the four waves in wave order.
// The pivot c of a stop is the mixture mean of the window's draw 0 there, a_0 that draw's own a.  A launch that holds draw 0
// (every device-entry call; the first chunk of the host entry) computes both in every block through the loop body every other
// draw goes through -- pass -2 with c = 0 gives c, pass -1 gives a_0, so a draw equal to draw 0 has b_d = a_d - a_0 = 0
// exactly -- and the block of slab 0 files them; later chunks of the host entry read them from there.
//
// Cost: 8 (3K + K^2) bytes read per draw against K^2 h_max + ~14 K n_h FMAs, one reciprocal, one division and one square root
// per (draw, horizon): HBM-bound at the production shape (K = 3, horizons (0, 12): 144 B per draw).
//
// Deterministic: a draw's thread and its place in that thread's sequence depend on the draw index alone; the butterfly and the
// wave order are fixed; the finalize kernel adds the slab sums in slab order.  No atomics.  Numerics: fp64 throughout; NaN
// inputs propagate (a draw past the end of the slab adds nothing).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mixmoments.hpp"
#include "stat_device.hpp"

namespace hmcg {

constexpr int MIX_NT = 256;                  // threads per block = draws per tile
constexpr int MIX_NW = MIX_NT / 64;
constexpr int MIX_FIN_NT = 64;
constexpr int MIX_ITEMS = hmcg_host::MIX_ITEMS;
constexpr int MIX_PIVOTS = hmcg_host::MIX_PIVOTS;

struct MixParams {
    const double* mu; const double* sig2; const double* pi_end; const double* A;
    double* part;                    // [W][nslab_total][n_h][MIX_ITEMS]
    double* piv;                     // [W][n_h][MIX_PIVOTS]: c, a_0
    long long nd, nd_ld;             // draws in this launch, leading dimension of the draw arrays
    long long nslab, slab0, nslab_total;     // slabs of this launch; its first slab and the slab count of the whole run
    int n_h, round5;
    int hz[HMCG_MAXH], slot[HMCG_MAXH];      // the ascending walk (mixmoments_plan.hpp)
};

// a[i] for a per-thread i without indexing the kernel arguments by a register (mixture_tile.hpp has the ladder inline, started at 0)
__device__ __forceinline__ int mix_pick(const int* a, int i)
{
    int r = a[0];
#pragma unroll
    for (int k = 1; k < HMCG_MAXH; ++k) r = i == k ? a[k] : r;
    return r;
}

template <int K, int NHC>
__global__ __launch_bounds__(MIX_NT) void mixmoments_kernel(const MixParams p)
{
    __shared__ double C[HMCG_MAXH], A0[HMCG_MAXH];      // per stop of the walk: the pivot and draw 0's a
    __shared__ double R[MIX_NW][NHC * MIX_ITEMS];
    const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
    HMCG_STAT_SLAB(w, s, dbeg, dend, p.nslab, p.nd);
    const int ntile = (int)((dend - dbeg + MIX_NT - 1) / MIX_NT);
    const double* mu = p.mu + (size_t)w * K * p.nd_ld;
    const double* sg = p.sig2 + (size_t)w * K * p.nd_ld;
    const double* pie = p.pi_end + (size_t)w * K * p.nd_ld;
    const double* At = p.A ? p.A + (size_t)w * K * K * p.nd_ld : nullptr;
    double* piv = p.piv + (size_t)w * (size_t)p.n_h * MIX_PIVOTS;
    const bool own_pivot = p.slab0 == 0;                // this launch's arrays start at the window's draw 0
    if (tid < p.n_h) {
        const int j = mix_pick(p.slot, tid);
        C[tid] = own_pivot ? 0.0 : piv[j * MIX_PIVOTS];
        A0[tid] = own_pivot ? 0.0 : piv[j * MIX_PIVOTS + 1];
    }
    __syncthreads();
    double acc[NHC][MIX_ITEMS];
#pragma unroll
    for (int i = 0; i < NHC; ++i)
#pragma unroll
        for (int e = 0; e < MIX_ITEMS; ++e) acc[i][e] = 0.0;
    // it = -2, -1: the pivot passes (thread 0 on draw 0), through the same code as every tile
#pragma unroll 1
    for (int it = own_pivot ? -2 : 0; it < ntile; ++it) {
        const auto [base, o, valid] = stat_tile(it, MIX_NT, tid, dbeg, dend);
        if (valid) {
            // every column is loaded before any is rounded: a rounding between two loads would make the second wait for the first
            double wv[K], m[K], v[K], a[K * K];
#pragma unroll
            for (int k = 0; k < K; ++k) wv[k] = (pie + (size_t)k * p.nd_ld + base)[o];
            if (At) {
#pragma unroll
                for (int c = 0; c < K * K; ++c) a[c] = (At + (size_t)c * p.nd_ld + base)[o];
            } else {
#pragma unroll
                for (int c = 0; c < K * K; ++c) a[c] = 0.0;
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                m[k] = (mu + (size_t)k * p.nd_ld + base)[o];
                v[k] = (sg + (size_t)k * p.nd_ld + base)[o];
            }
            if (p.round5) {                                      // stat_in of stat_device.hpp, taken once for all cells
#pragma unroll
                for (int k = 0; k < K; ++k) { wv[k] = round5(wv[k]); m[k] = round5(m[k]); v[k] = round5(v[k]); }
#pragma unroll
                for (int c = 0; c < K * K; ++c) a[c] = round5(a[c]);
            }
            int step = 0;
#pragma unroll
            for (int i = 0; i < NHC; ++i) {
                if (i < p.n_h) {
                    if (At) {
#pragma unroll 1
                        for (; step < p.hz[i]; ++step) HMCG_OMEGA_STEP(K, wv, a, 1);
                    }
                    const double c = C[i], a0 = A0[i];
                    double sw = wv[0];
#pragma unroll
                    for (int k = 1; k < K; ++k) sw += wv[k];
                    double p1 = 0.0, p2 = 0.0, p3 = 0.0, p4 = 0.0;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const double d = m[k] - c, d2 = d * d, vk = v[k];
                        p1 = fma(wv[k], d, p1);
                        p2 = fma(wv[k], d2 + vk, p2);
                        p3 = fma(wv[k], d * fma(3.0, vk, d2), p3);
                        p4 = fma(wv[k], fma(d2, fma(6.0, vk, d2), 3.0 * vk * vk), p4);
                    }
                    const double rs = 1.0 / sw, am = p1 * rs;
                    double u2 = 0.0, u3 = 0.0;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const double e = (m[k] - c) - am, e2 = e * e, vk = v[k];
                        u2 = fma(wv[k], e2 + vk, u2);
                        u3 = fma(wv[k], e * fma(3.0, vk, e2), u3);
                    }
                    const double var = u2 * rs;
                    const double sk = (u3 * rs) / (var * sqrt(var));
                    const double b = am - a0;
                    if (it == -2) C[i] = am;
                    else if (it == -1) A0[i] = am;
                    else {
                        acc[i][0] += sw; acc[i][1] += p1; acc[i][2] += p2; acc[i][3] += p3; acc[i][4] += p4;
                        acc[i][5] += b; acc[i][6] = fma(b, b, acc[i][6]); acc[i][7] += var; acc[i][8] += sk;
                    }
                }
            }
        }
        if (it < 0) __syncthreads();
    }
    if (own_pivot && s == 0 && tid < p.n_h) {
        const int j = mix_pick(p.slot, tid);
        piv[j * MIX_PIVOTS] = C[tid];
        piv[j * MIX_PIVOTS + 1] = A0[tid];
    }
#pragma unroll
    for (int i = 0; i < NHC; ++i) {
        if (i < p.n_h) {
#pragma unroll
            for (int e = 0; e < MIX_ITEMS; ++e) {
                double t = acc[i][e];
                HMCG_WAVE_SUM(t);
                if (lane == 0) R[q][i * MIX_ITEMS + e] = t;
            }
        }
    }
    __syncthreads();
    if (tid < p.n_h * MIX_ITEMS) {
        const int i = tid / MIX_ITEMS, e = tid - i * MIX_ITEMS;
        double t = R[0][tid];
#pragma unroll
        for (int x = 1; x < MIX_NW; ++x) t += R[x][tid];
        double* row = p.part + HMCG_STAT_ROW(w, p.nslab_total, p.slab0 + s, p.n_h * MIX_ITEMS);
        row[mix_pick(p.slot, i) * MIX_ITEMS + e] = t;
    }
}

// One block per window, thread j on horizon j: the slab sums in slab order, then the table of include/hmcg.h.
__global__ __launch_bounds__(MIX_FIN_NT) void mixmoments_finalize_kernel(const double* part, const double* piv, double* out,
                                                                       long long nslab, int n_h, double n)
{
    const int w = blockIdx.x, j = threadIdx.x;
    if (j >= n_h) return;
    const double* col = part + ((size_t)w * (size_t)nslab * (size_t)n_h + (size_t)j) * MIX_ITEMS;
    double T[MIX_ITEMS];
#pragma unroll
    for (int e = 0; e < MIX_ITEMS; ++e) T[e] = 0.0;
    for (long long sl = 0; sl < nslab; ++sl) {                   // HMCG_SLAB_SUM of stat_device.hpp, nine items per trip
#pragma unroll
        for (int e = 0; e < MIX_ITEMS; ++e) T[e] += col[(size_t)sl * (size_t)(n_h * MIX_ITEMS) + e];
    }
    const double c = piv[((size_t)w * (size_t)n_h + (size_t)j) * MIX_PIVOTS];
    const double m1 = T[1] / T[0], m2 = T[2] / T[0], m3 = T[3] / T[0], m4 = T[4] / T[0];
    const double m11 = m1 * m1;
    const double var = m2 - m11;
    double* o = out + ((size_t)w * (size_t)n_h + (size_t)j) * HMCG_MIX_STRIDE;
    o[0] = c + m1;
    o[1] = var;
    o[2] = (m3 - 3.0 * m1 * m2 + 2.0 * m11 * m1) / (var * sqrt(var));
    o[3] = (m4 - 4.0 * m1 * m3 + 6.0 * m11 * m2 - 3.0 * m11 * m11) / (var * var) - 3.0;
    o[4] = T[7] / n;
    const double q1 = T[5] / n;
    o[5] = T[6] / n - q1 * q1;
    o[6] = T[8] / n;
    o[7] = T[0] / n;
}

}  // namespace hmcg

namespace hmcg_host {

size_t mix_part_doubles(int W, long long nd, int n_h)
{
    return (size_t)W * (size_t)n_h * ((size_t)pred_slabs(nd) * (size_t)MIX_ITEMS + (size_t)MIX_PIVOTS);
}

hipError_t launch_mixmoments(const MixArgs& a, hipStream_t stream)
{
    if (a.W <= 0 || a.nd <= 0) return hipSuccess;
    if (a.K < 2 || a.K > HMCG_MAXK || a.n_h < 1 || a.n_h > HMCG_MAXH) return hipErrorInvalidValue;
    hmcg::MixParams p{};
    bool with_A = false;
    for (int i = 0; i < HMCG_MAXH; ++i) {
        p.hz[i] = i < a.n_h ? a.walk.hz[i] : 0;
        p.slot[i] = i < a.n_h ? a.walk.slot[i] : 0;
        if (p.hz[i] < 0 || p.slot[i] < 0 || p.slot[i] >= a.n_h || (i > 0 && i < a.n_h && p.hz[i] < p.hz[i - 1])) return hipErrorInvalidValue;
        with_A = with_A || p.hz[i] > 0;
    }
    if (with_A && !a.A) return hipErrorInvalidValue;
    p.mu = a.mu; p.sig2 = a.sig2; p.pi_end = a.pi_end; p.A = with_A ? a.A : nullptr;
    p.part = a.part; p.piv = a.part + (size_t)a.W * (size_t)a.nslab_total * (size_t)a.n_h * (size_t)MIX_ITEMS;
    p.nd = a.nd; p.nd_ld = a.nd_ld; p.nslab = pred_slabs(a.nd); p.slab0 = a.slab0; p.nslab_total = a.nslab_total;
    p.n_h = a.n_h; p.round5 = a.round5 ? 1 : 0;
    if (!slab_range_ok(a.W, a.nd, a.nd_ld, a.slab0, a.nslab_total)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((long long)a.W * p.nslab)), block(hmcg::MIX_NT);
    // two builds per K: accumulators for up to 2 stops of the walk (the production call: horizons 0 and 12) and for up to HMCG_MAXH
#define HMCG_MIX(K_)                                                                                              \
    if (a.n_h <= 2) hipLaunchKernelGGL((hmcg::mixmoments_kernel<K_, 2>), grid, block, 0, stream, p);              \
    else hipLaunchKernelGGL((hmcg::mixmoments_kernel<K_, HMCG_MAXH>), grid, block, 0, stream, p)
    HMCG_SWITCH_K(a.K, HMCG_MIX)
#undef HMCG_MIX
    return hipGetLastError();
}

hipError_t launch_mixmoments_finalize(const double* part, double* out, int W, int n_h, long long nd_total, hipStream_t stream)
{
    if (W <= 0) return hipSuccess;
    if (n_h < 1 || n_h > HMCG_MAXH) return hipErrorInvalidValue;
    const long long nslab = pred_slabs(nd_total);
    const double* piv = part + (size_t)W * (size_t)nslab * (size_t)n_h * (size_t)MIX_ITEMS;
    hipLaunchKernelGGL(hmcg::mixmoments_finalize_kernel, dim3((unsigned)W), dim3(hmcg::MIX_FIN_NT), 0, stream, part, piv, out, nslab, n_h,
                       (double)nd_total);
    return hipGetLastError();
}

}  // namespace hmcg_host
