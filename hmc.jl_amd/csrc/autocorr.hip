// autocorr.hip -- autocovariances, integrated autocorrelation time, effective sample size, Monte-Carlo standard error and
// split-R-hat of a window's draws, on the device.  No reference script computes them; they are what tells a user how many of the
// 250 000 kept sweeps of a window are worth anything.  The rules stand in include/hmcg.h.
//
// Shape.
//   accumulate kernel  one block of 256 threads per (window, column); it walks the launch's 1024-draw slabs in order.  The slab's
//                      a_d = x'_d - p and the lags_r draws before it stand in LDS (index i at i + i / 8: one pad per eight doubles,
//                      so that lanes eight doubles apart fall into different banks).  A thread holds ACF_J = 8 adjacent lags and
//                      one share of the slab's draws (autocorr_plan.hpp) and walks its draws in register tiles of eight: eight
//                      broadcast reads of a_d .. a_d+7 and eight reads of the next a_(d - l0) .. feed 64 FMAs, the older half of
//                      the 15-value window stays in registers.  The shares of a lag are added in share order through LDS and the
//                      slab's sum joins the lag's running sum, which its owner thread keeps in a register across the slabs.
//                      The global loads of the next slab are issued before the arithmetic of the current one.  S1 and S2 of the
//                      thirds [0, h), [h, n - h), [n - h, n) go through a fixed butterfly per slab (squares unfused, so numpy
//                      can restate them bit for bit) into six running sums; the first and last L values of a into the work area.
//   finalize kernel    one block per (window, column): thread 0 takes the running edge sums H_l, T_l, all threads acov_l, thread 0
//                      Geyer's sequence and the split-R-hat; no operation there may fuse.
//
// Deterministic: the split of a slab depends on L alone, the slabs on nd alone; no atomics.  A launch that holds draw 0 starts
// the running sums and files the pivot; later launches (chunks of the host entry) continue from the work area.
// Numerics: fp64; products with a draw before the chain's first or behind its last are taken with 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "autocorr.hpp"
#include "stat_device.hpp"

namespace hmcg {

using hmcg_host::PRED_SLAB;
using hmcg_host::ACF_NT;
using hmcg_host::ACF_J;
using hmcg_host::ACF_SUMS;

constexpr int AC_NW = ACF_NT / 64;
constexpr int AC_SLAB = (int)PRED_SLAB;
constexpr int AC_HALO_MAX = (HMCG_ACF_MAXLAG + ACF_J) / ACF_J * ACF_J;          // lags_r at the largest L
constexpr int AC_STAGE = AC_SLAB + AC_HALO_MAX;                                   // staged draws at most
constexpr int AC_LOADS = (AC_STAGE + ACF_NT - 1) / ACF_NT;                        // per thread
constexpr int AC_TILES = AC_SLAB / ACF_NT;
constexpr int AC_OWN = (HMCG_ACF_MAXLAG + ACF_NT) / ACF_NT;                       // running lag sums per thread
constexpr int AC_RED = ACF_J + 1;                                                 // stride of a thread's share sums in LDS

struct AcfParams {
    const double* x;
    double* work;
    double* acov;
    double* diag;
    long long d_origin, n, pre, nd, ld;
    int W, C, L, round5;
};

__device__ __forceinline__ int ac_pos(int i) { return i + (i >> 3); }

__device__ __forceinline__ double ac_sq(double v)
{
#pragma clang fp contract(off)
    const double s = v * v;
    return s;
}

__global__ __launch_bounds__(ACF_NT) void autocorr_accumulate_kernel(const AcfParams p)
{
    __shared__ double st[AC_STAGE + AC_STAGE / 8 + 8];
    __shared__ double red[ACF_NT * AC_RED];
    __shared__ double sred[AC_NW][ACF_SUMS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const hmcg_host::AcfPlan pl = hmcg_host::acf_plan(p.L);
    const int lt = tid & (pl.lag_threads - 1), g = tid / pl.lag_threads;
    const int l0 = lt * ACF_J;
    const bool active = l0 <= p.L;
    const size_t wc = blockIdx.x;
    const double* col = p.x + wc * (size_t)p.ld;
    double* wk = p.work + wc * (size_t)hmcg_host::acf_work_doubles(p.L);
    double* w_acc = wk;
    double* w_sums = wk + (p.L + 1);
    double* w_piv = w_sums + ACF_SUMS;
    double* w_edge = w_piv + 1;
    const bool first = p.d_origin == 0;
    double pvt;
    if (first) {
        const double f = col[p.pre];                     // pre == 0 here
        pvt = stat_in(f, p.round5);
    } else pvt = *w_piv;
    const long long nslab = (p.n + PRED_SLAB - 1) / PRED_SLAB;
    const long long dend = p.d_origin + p.n;             // one past this launch's last draw
    const long long h = p.nd / 2;

    double run[AC_OWN];
#pragma unroll
    for (int i = 0; i < AC_OWN; ++i) {
        const int l = tid + ACF_NT * i;
        run[i] = (!first && l <= p.L) ? w_acc[l] : 0.0;
    }
    double rs = (!first && tid < ACF_SUMS) ? w_sums[tid] : 0.0;

    double v[AC_LOADS];
    const int nstage = AC_SLAB + pl.lags_r;
    // the draws of slab s and its halo, as far as they exist: position i holds run draw sd0 - lags_r + i
    auto fetch = [&](long long s) {
        const long long sd0 = p.d_origin + s * PRED_SLAB;
        const long long lo = sd0 - p.L > 0 ? sd0 - p.L : 0;
#pragma unroll
        for (int k = 0; k < AC_LOADS; ++k) {
            const int i = tid + ACF_NT * k;
            const long long d = sd0 - pl.lags_r + i;
            v[k] = (i < nstage && d >= lo && d < dend) ? col[d - p.d_origin + p.pre] : 0.0;
        }
    };
    auto stage = [&](long long s) {
        const long long sd0 = p.d_origin + s * PRED_SLAB;
        const long long lo = sd0 - p.L > 0 ? sd0 - p.L : 0;
#pragma unroll
        for (int k = 0; k < AC_LOADS; ++k) {
            const int i = tid + ACF_NT * k;
            const long long d = sd0 - pl.lags_r + i;
            if (i < nstage) {
                const double xr = stat_in(v[k], p.round5);
                st[ac_pos(i)] = (d >= lo && d < dend) ? xr - pvt : 0.0;
            }
        }
    };

    fetch(0);
    stage(0);
    __syncthreads();
#pragma unroll 1
    for (long long s = 0; s < nslab; ++s) {
        const long long sd0 = p.d_origin + s * PRED_SLAB;
        if (s + 1 < nslab) fetch(s + 1);                 // in flight during the arithmetic below

        double acc[ACF_J];
#pragma unroll
        for (int j = 0; j < ACF_J; ++j) acc[j] = 0.0;
        if (active) {
            const int r0 = g * pl.group_draws;
            const double* ad_p = st + ac_pos(pl.lags_r + r0);
            const double* win_p = st + ac_pos(pl.lags_r + r0 - l0 - ACF_J);
            double win[2 * ACF_J], ad[ACF_J];            // a_(d0 - l0 - 8) .. a_(d0 - l0 + 7) of the tile that starts at draw d0
#pragma unroll
            for (int k = 0; k < ACF_J; ++k) win[ACF_J + k] = win_p[k];
#pragma unroll 1
            for (int t = 0; t < pl.group_draws / ACF_J; ++t) {
                win_p += ACF_J + 1;
#pragma unroll
                for (int k = 0; k < ACF_J; ++k) { win[k] = win[ACF_J + k]; win[ACF_J + k] = win_p[k]; ad[k] = ad_p[k]; }
                ad_p += ACF_J + 1;
#pragma unroll
                for (int k = 0; k < ACF_J; ++k) {        // draw d0 + k with lag l0 + j: a_(d0 - l0 + k - j)
#pragma unroll
                    for (int j = 0; j < ACF_J; ++j) acc[j] = fma(ad[k], win[ACF_J + k - j], acc[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < ACF_J; ++j) red[tid * AC_RED + j] = acc[j];

        // S1, S2 of the slab's draws in each third of the chain
        double sm[ACF_SUMS];
#pragma unroll
        for (int e = 0; e < ACF_SUMS; ++e) sm[e] = 0.0;
#pragma unroll
        for (int k = 0; k < AC_TILES; ++k) {
            const int r = tid + ACF_NT * k;
            const long long d = sd0 + r;
            const double a = st[ac_pos(pl.lags_r + r)];
            const int third = d < h ? 0 : (d < p.nd - h ? 1 : 2);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const double u = third == q ? a : 0.0;
                const double sq = ac_sq(u);
                sm[2 * q] = sm[2 * q] + u;
                sm[2 * q + 1] = sm[2 * q + 1] + sq;
            }
        }
#pragma unroll
        for (int e = 0; e < ACF_SUMS; ++e) {
            HMCG_WAVE_SUM(sm[e]);
            if (lane == 0) sred[wv][e] = sm[e];
        }

        // the first and the last L values of a
        if (sd0 == 0)
            for (int i = tid; i < p.L; i += ACF_NT) w_edge[i] = st[ac_pos(pl.lags_r + i)];
        if (sd0 + PRED_SLAB >= p.nd)
            for (int k = tid; k < p.L; k += ACF_NT) w_edge[p.L + k] = st[ac_pos(pl.lags_r + (int)(p.nd - 1 - k - sd0))];
        __syncthreads();

#pragma unroll
        for (int i = 0; i < AC_OWN; ++i) {
            const int l = tid + ACF_NT * i;
            if (l <= p.L) {
                const double* src = red + (l >> 3) * AC_RED + (l & 7);
                double t = src[0];
                for (int q = 1; q < pl.groups; ++q) t += src[q * pl.lag_threads * AC_RED];
                run[i] += t;
            }
        }
        if (tid < ACF_SUMS) {
            double t = sred[0][tid];
#pragma unroll
            for (int q = 1; q < AC_NW; ++q) t += sred[q][tid];
            rs += t;
        }
        __syncthreads();
        if (s + 1 < nslab) {
            stage(s + 1);
            __syncthreads();
        }
    }
#pragma unroll
    for (int i = 0; i < AC_OWN; ++i) {
        const int l = tid + ACF_NT * i;
        if (l <= p.L) w_acc[l] = run[i];
    }
    if (tid < ACF_SUMS) w_sums[tid] = rs;
    if (first && tid == 0) *w_piv = pvt;
}

// One block per (window, column).
__global__ __launch_bounds__(ACF_NT) void autocorr_finalize_kernel(const AcfParams p)
{
#pragma clang fp contract(off)
    __shared__ double eh[HMCG_ACF_MAXLAG + 1], et[HMCG_ACF_MAXLAG + 1], ac[HMCG_ACF_MAXLAG + 1];
    const int tid = threadIdx.x;
    const size_t wc = blockIdx.x;
    const double* wk = p.work + wc * (size_t)hmcg_host::acf_work_doubles(p.L);
    const double* w_acc = wk;
    const double* w_sums = wk + (p.L + 1);
    const double pvt = w_sums[ACF_SUMS];
    const double* w_edge = w_sums + ACF_SUMS + 1;
    for (int i = tid; i < p.L; i += ACF_NT) { eh[i + 1] = w_edge[i]; et[i + 1] = w_edge[p.L + i]; }
    __syncthreads();
    if (tid == 0) {
        double H = 0.0, T = 0.0;
        eh[0] = 0.0; et[0] = 0.0;
        for (int l = 1; l <= p.L; ++l) {
            H = H + eh[l];
            T = T + et[l];
            eh[l] = H;
            et[l] = T;
        }
    }
    __syncthreads();
    const double n = (double)p.nd;
    const double s1a = w_sums[0] + w_sums[2];
    const double S1 = s1a + w_sums[4];
    const double s2a = w_sums[1] + w_sums[3];
    const double S2 = s2a + w_sums[5];
    const double m = S1 / n;
    const double twoS1 = 2.0 * S1;
    for (int l = tid; l <= p.L; l += ACF_NT) {
        const double q1 = twoS1 - eh[l];
        const double q = q1 - et[l];
        const double mq = m * q;
        const double r = w_acc[l] - mq;
        const double nl = (double)(p.nd - l);
        const double s0 = nl * m;
        const double s = s0 * m;
        const double t = r + s;
        const double a = t / n;
        ac[l] = a;
        p.acov[wc * (size_t)(p.L + 1) + (size_t)l] = a;
    }
    __syncthreads();
    if (tid != 0) return;
    const double nan = stat_nan();
    const double sq = S1 * S1;
    const double corr = sq / n;
    const double dv = S2 - corr;
    const double variance = dv / (n - 1.0);
    double tau = nan, ess = nan, mcse = nan;
    int pairs = 0, truncated = 0;
    const double a0 = ac[0];
    if (a0 > 0.0) {
        const int np = (p.L + 1) / 2;
        double ta = -1.0, prev = __longlong_as_double(0x7ff0000000000000ll);
        int k = 0;
        for (; k < np; ++k) {
            const double ra = ac[2 * k] / a0;
            const double rb = ac[2 * k + 1] / a0;
            double P = ra + rb;
            if (!(P > 0.0)) break;
            if (P > prev) P = prev;
            const double P2 = 2.0 * P;
            ta = ta + P2;
            prev = P;
        }
        pairs = k;
        truncated = k == np ? 1 : 0;
        if (pairs > 0) tau = ta;
        ess = n / tau;
        const double vt = variance * tau;
        const double vn = vt / n;
        mcse = sqrt(vn);
    }
    const double hh = (double)(p.nd / 2);
    const double m1 = w_sums[0] / hh, m2 = w_sums[4] / hh;
    const double sq1 = w_sums[0] * w_sums[0], sq2 = w_sums[4] * w_sums[4];
    const double c1 = sq1 / hh, c2 = sq2 / hh;
    const double d1 = w_sums[1] - c1, d2 = w_sums[5] - c2;
    const double hm1 = hh - 1.0;
    const double v1 = d1 / hm1, v2 = d2 / hm1;
    const double vs = v1 + v2;
    const double Wv = vs / 2.0;
    const double fr = hm1 / hh;
    const double t1 = fr * Wv;
    const double dm = m1 - m2;
    const double dm2 = dm * dm;
    const double t2 = dm2 / 2.0;
    const double mid = w_sums[2] - w_sums[2];            // 0, or NaN when the middle draw of an odd n is not finite
    const double vp = t1 + t2;
    const double varplus = vp + mid;
    const double ratio = varplus / Wv;
    const double rhat = sqrt(ratio);
    double* o = p.diag + wc * HMCG_ACF_STRIDE;
    o[0] = pvt + m;
    o[1] = variance;
    o[2] = tau;
    o[3] = ess;
    o[4] = mcse;
    o[5] = (double)pairs;
    o[6] = (double)truncated;
    o[7] = rhat;
}

}  // namespace hmcg

namespace hmcg_host {

size_t acf_work_bytes(int W, int C, int L) { return sizeof(double) * (size_t)W * (size_t)C * (size_t)acf_work_doubles(L); }

static bool acf_params(const AcfArgs& a, hmcg::AcfParams& p)
{
    if (a.W < 1 || a.C < 1 || a.C > HMCG_MAXK * HMCG_MAXK || (long long)a.W * a.C > 0x7fffffffLL) return false;
    if (a.L < 0 || a.L > HMCG_ACF_MAXLAG || a.nd < 1 || (long long)a.L > a.nd - 1) return false;
    if (!chunk_origin_ok(a.d_origin, a.n, a.nd)) return false;
    if (a.pre != acf_pre(a.d_origin, a.L) || a.ld < a.pre + a.n) return false;
    if (!a.x || !a.work || !a.acov || !a.diag) return false;
    p = hmcg::AcfParams{};
    p.x = a.x; p.work = reinterpret_cast<double*>(a.work); p.acov = a.acov; p.diag = a.diag;
    p.d_origin = a.d_origin; p.n = a.n; p.pre = a.pre; p.nd = a.nd; p.ld = a.ld;
    p.W = a.W; p.C = a.C; p.L = a.L; p.round5 = a.round5 ? 1 : 0;
    return true;
}

hipError_t launch_autocorr_accumulate(const AcfArgs& a, hipStream_t stream)
{
    hmcg::AcfParams p;
    if (!acf_params(a, p)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hmcg::autocorr_accumulate_kernel, dim3((unsigned)((long long)a.W * a.C)), dim3(ACF_NT), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_autocorr_finalize(const AcfArgs& a, hipStream_t stream)
{
    hmcg::AcfParams p;
    if (!acf_params(a, p)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hmcg::autocorr_finalize_kernel, dim3((unsigned)((long long)a.W * a.C)), dim3(ACF_NT), 0, stream, p);
    return hipGetLastError();
}

}  // namespace hmcg_host
