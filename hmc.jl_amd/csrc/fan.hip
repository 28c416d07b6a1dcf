// fan.hip -- quantiles of the predictive regime mixture, per window, horizon and probability, on the device: the fan chart.
//
// What it adds (joe5saia/Hmc.jl): code/hassan_cdfs/calc_cdfs.jl evaluates the pooled CDF of a window's nd * K normals on a fixed
// grid and `finverse` reads a quantile off that grid; a forecaster reports the median, the 68 % and 95 % bands and value-at-risk
// levels, which need the CDF where the quantile lies, to full precision.  Here the CDF of predictive.hip is inverted by grid
// refinement (include/hmcg_fan.h states the algorithm, fan_plan.hpp holds its arithmetic outside the CDF): a range pass, round 1
// with 129 points per (window, horizon) shared by every probability, then rounds of 31 interior points per (window, horizon,
// probability), each dividing the bracket by 32.  Between two rounds the brackets live in `out` in HBM; nothing is read back.
//
// fan_eval_kernel is the tile of predictive_cdf_kernel (mixture_tile.hpp): one block per (window, slab of PRED_SLAB draws, 128
// items), a tile of 64 draws staged in LDS as (mu, c) pairs with the weights of every horizon, each thread walking the tile in
// draw order with ITS point: an item is (horizon, point) in round 1 and (horizon, probability, point) later, and its y comes from
// the bracket table -- range[w] in round 1, out[w][j][i] later -- not from a grid.  Both kernels expand the one walk, so an F
// computed here carries the bits hmcg_predictive_cdf gives for the same point.
// fan_step_kernel, one block per (window, horizon): a thread per item adds the slab sums in slab order and divides by nd, then
// a thread per probability chooses its cell and writes the next bracket; after the last round also q and the flag.
// fan_range_kernel / fan_range_finalize_kernel: per-slab fmin / fmax of mu -+ 40 sd, then over the slabs.
// Deterministic: no atomics anywhere; fmin / fmax do not depend on the order.  fp64 throughout, no scratch, no inline assembly.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fan.hpp"
#include "mixture_tile.hpp"

namespace hmcg {

using hmcg_host::FAN_M;
using hmcg_host::FAN_M1;

constexpr int FAN_RANGE_NT = 256;
constexpr int FAN_STEP_NT = 256;
constexpr int FAN_STEP_F = HMCG_FAN_MAXP * (FAN_M - 1);      // 496 >= 129: the most items of one (window, horizon)
static_assert(FAN_STEP_F >= FAN_M1 + 1, "the step kernel's F table holds round 1 too");

struct FanRangeParams {
    const double* mu; const double* sig2;
    double* part;                    // [W][nslab_total][rowlen], (min, max) in the first two of a row
    double* range;                   // [W][2]
    long long nd, nd_ld, nslab, slab0, nslab_total;
    int K, rowlen, round5;
};

__global__ __launch_bounds__(FAN_RANGE_NT) void fan_range_kernel(const FanRangeParams p)
{
    __shared__ double R[2][FAN_RANGE_NT / 64];
    const int tid = threadIdx.x;
    HMCG_STAT_SLAB(w, s, dbeg, dend, p.nslab, p.nd);
    const double* mu = p.mu + (size_t)w * p.K * p.nd_ld;
    const double* sg = p.sig2 + (size_t)w * p.K * p.nd_ld;
    double lo = stat_nan(), hi = stat_nan();
    for (int k = 0; k < p.K; ++k)
        for (long long d = dbeg + tid; d < dend; d += FAN_RANGE_NT) {
            const size_t off = (size_t)k * p.nd_ld + (size_t)d;
            double l, h;
            hmcg_host::fan_reach(stat_in(mu[off], p.round5), stat_in(sg[off], p.round5), &l, &h);
            lo = fmin(lo, l);
            hi = fmax(hi, h);
        }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, m, 64));
        hi = fmax(hi, __shfl_xor(hi, m, 64));
    }
    if ((tid & 63) == 0) { R[0][tid >> 6] = lo; R[1][tid >> 6] = hi; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int q = 1; q < FAN_RANGE_NT / 64; ++q) { lo = fmin(lo, R[0][q]); hi = fmax(hi, R[1][q]); }
        double* row = p.part + HMCG_STAT_ROW(w, p.nslab_total, p.slab0 + s, p.rowlen);
        row[0] = lo;
        row[1] = hi;
    }
}

__global__ __launch_bounds__(64) void fan_range_finalize_kernel(const double* part, double* range, long long nslab, int rowlen, int W)
{
    const int w = (int)blockIdx.x * 64 + threadIdx.x;
    if (w >= W) return;
    const double* row = part + HMCG_STAT_ROW(w, nslab, 0, rowlen);
    double lo = stat_nan(), hi = stat_nan();
    for (long long sl = 0; sl < nslab; ++sl) {
        lo = fmin(lo, row[(size_t)sl * (size_t)rowlen]);
        hi = fmax(hi, row[(size_t)sl * (size_t)rowlen + 1]);
    }
    range[2 * (size_t)w] = lo;
    range[2 * (size_t)w + 1] = hi;
}

struct FanEvalParams {
    const double* mu; const double* sig2; const double* pi_end; const double* A;
    const double* tab;               // the brackets: round 1 range [W][2], later out [W][n_h][n_p][5] with (lo, hi) at 1, 2
    double* part;                    // [W][nslab_total][rowlen]
    long long nd, nd_ld;             // draws in this launch, leading dimension of the draw arrays
    long long nslab, slab0, nslab_total;     // slabs of this launch; its first slab and the slab count of the whole run
    int n_h, n_p, items, items_h, rowlen, first, round5;
    int hz[HMCG_MAXH];
};

template <int K>
__global__ __launch_bounds__(MIXTILE_NT) void fan_eval_kernel(const FanEvalParams p)
{
    extern __shared__ double fan_lds[];
    const int n_h = p.n_h;
    HMCG_MIX_TILE_LDS(K, fan_lds, n_h, MC, Ws, As);
    const int tid = threadIdx.x;
    HMCG_STAT_SLAB(w, s, dbeg, dend, p.nslab, p.nd);
    const int e = (int)blockIdx.y * MIXTILE_NT + tid;    // this thread's item: horizon j, then the point within it
    const bool live = e < p.items;
    const int j = live ? e / p.items_h : 0, l = live ? e - j * p.items_h : 0;
    double y;
    if (p.first) {
        const double* b = p.tab + 2 * (size_t)w;
        y = hmcg_host::fan_point(b[0], b[1], FAN_M1, l);
    } else {
        const int i = l / (FAN_M - 1), m = l - i * (FAN_M - 1) + 1;
        const double* b = p.tab + HMCG_FAN_STRIDE * (((size_t)w * n_h + j) * p.n_p + i);
        y = hmcg_host::fan_point(b[1], b[2], FAN_M, m);
    }
    const double* mu = p.mu + (size_t)w * K * p.nd_ld;
    const double* sig2 = p.sig2 + (size_t)w * K * p.nd_ld;
    const double* pie = p.pi_end + (size_t)w * K * p.nd_ld;
    const double* At = p.A ? p.A + (size_t)w * K * K * p.nd_ld : nullptr;
    double acc = 0.0;
#define FAN_DRAW(dd) (size_t)(d0 + (dd))
    for (long long d0 = dbeg; d0 < dend; d0 += MIXTILE_TD) {
        const int nv = dend - d0 < MIXTILE_TD ? (int)(dend - d0) : MIXTILE_TD;
        HMCG_MIX_TILE_STAGE(K, MC, Ws, As, mu, sig2, pie, At, p, FAN_DRAW, nv, n_h, tid);
        if (live) HMCG_MIX_TILE_WALK(K, MC, Ws, nv, n_h, j, y, acc);
        __syncthreads();
    }
#undef FAN_DRAW
    if (live) p.part[HMCG_STAT_ROW(w, p.nslab_total, p.slab0 + s, p.rowlen) + (size_t)e] = acc;
}

struct FanStepParams {
    const double* part;              // [W][nslab][rowlen]
    const double* range;             // [W][2]
    double* out;                     // [W][n_h][n_p][5]
    int32_t* flag;                   // [W][n_h][n_p]
    long long nslab;
    double nd;
    int n_h, n_p, items_h, rowlen, first, last;
    double probs[HMCG_FAN_MAXP];
};

__global__ __launch_bounds__(FAN_STEP_NT) void fan_step_kernel(const FanStepParams p)
{
    __shared__ double Fs[FAN_STEP_F];
    const int tid = threadIdx.x;
    const int w = (int)blockIdx.x / p.n_h, j = (int)blockIdx.x - w * p.n_h;
    for (int e = tid; e < p.items_h; e += FAN_STEP_NT) {
        const double* col = p.part + HMCG_STAT_ROW(w, p.nslab, 0, p.rowlen) + (size_t)(j * p.items_h + e);
        HMCG_SLAB_SUM(sum, col, p.nslab, p.rowlen);
        Fs[e] = sum / p.nd;
    }
    __syncthreads();
    if (tid >= p.n_p) return;
    const int i = tid;
    double pr = 0.0;
#pragma unroll
    for (int q = 0; q < HMCG_FAN_MAXP; ++q) pr = i == q ? p.probs[q] : pr;
    double* o = p.out + HMCG_FAN_STRIDE * (((size_t)w * p.n_h + j) * p.n_p + i);
    double b[4];
    if (p.first) {
        b[0] = p.range[2 * (size_t)w]; b[1] = p.range[2 * (size_t)w + 1]; b[2] = 0.0; b[3] = 0.0;
        hmcg_host::fan_choose(b, Fs, true, pr);
    } else {
        b[0] = o[1]; b[1] = o[2]; b[2] = o[3]; b[3] = o[4];
        hmcg_host::fan_choose(b, Fs + i * (FAN_M - 1), false, pr);
    }
    o[1] = b[0]; o[2] = b[1]; o[3] = b[2]; o[4] = b[3];
    if (p.last) {
        double q;
        const int fl = hmcg_host::fan_finish(b, pr, &q);
        o[0] = q;
        p.flag[((size_t)w * p.n_h + j) * p.n_p + i] = fl;
    }
}

}  // namespace hmcg

namespace hmcg_host {

hipError_t launch_fan_range(const FanArgs& a, hipStream_t stream)
{
    if (a.W <= 0 || a.nd <= 0) return hipSuccess;
    if (!slab_range_ok(a.W, a.nd, a.nd_ld, a.slab0, a.nslab_total)) return hipErrorInvalidValue;
    hmcg::FanRangeParams p{};
    p.mu = a.mu; p.sig2 = a.sig2; p.part = a.part; p.range = a.range;
    p.nd = a.nd; p.nd_ld = a.nd_ld; p.nslab = pred_slabs(a.nd); p.slab0 = a.slab0; p.nslab_total = a.nslab_total;
    p.K = a.K; p.rowlen = fan_max_items(a.n_h, a.n_p); p.round5 = a.round5 ? 1 : 0;
    hipLaunchKernelGGL(hmcg::fan_range_kernel, dim3((unsigned)((long long)a.W * p.nslab)), dim3(hmcg::FAN_RANGE_NT), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_fan_range_finalize(const FanArgs& a, hipStream_t stream)
{
    if (a.W <= 0) return hipSuccess;
    hipLaunchKernelGGL(hmcg::fan_range_finalize_kernel, dim3((unsigned)((a.W + 63) / 64)), dim3(64), 0, stream, a.part, a.range, a.nslab_total,
                       fan_max_items(a.n_h, a.n_p), a.W);
    return hipGetLastError();
}

hipError_t launch_fan_eval(const FanArgs& a, int round, hipStream_t stream)
{
    if (a.W <= 0 || a.nd <= 0) return hipSuccess;
    const bool first = round == 1;
    hmcg::FanEvalParams p{};
    p.mu = a.mu; p.sig2 = a.sig2; p.pi_end = a.pi_end; p.A = a.A; p.tab = first ? a.range : a.out; p.part = a.part;
    p.nd = a.nd; p.nd_ld = a.nd_ld; p.nslab = pred_slabs(a.nd); p.slab0 = a.slab0; p.nslab_total = a.nslab_total;
    p.n_h = a.n_h; p.n_p = a.n_p; p.items_h = fan_items_h(a.n_p, first); p.items = fan_items(a.n_h, a.n_p, first);
    p.rowlen = fan_max_items(a.n_h, a.n_p); p.first = first ? 1 : 0; p.round5 = a.round5 ? 1 : 0;
    const bool with_A = fill_horizons(a.n_h, a.horizons, p.hz);
    if (with_A && !a.A) return hipErrorInvalidValue;
    if (!with_A) p.A = nullptr;
    // nd_ld >= nd is part of the rule; check_fan has enforced it ahead of every launch already
    if (!slab_range_ok(a.W, a.nd, a.nd_ld, a.slab0, a.nslab_total)) return hipErrorInvalidValue;
    const size_t lds = mixture_lds_bytes(a.K, a.n_h, with_A);
    const dim3 grid((unsigned)((long long)a.W * p.nslab), (unsigned)((p.items + hmcg::MIXTILE_NT - 1) / hmcg::MIXTILE_NT)), block(hmcg::MIXTILE_NT);
#define HMCG_FAN_EVAL(K_) HMCG_LAUNCH_LDS(hmcg::fan_eval_kernel<K_>, grid, block, lds, stream, p)
    HMCG_SWITCH_K(a.K, HMCG_FAN_EVAL)
#undef HMCG_FAN_EVAL
    return hipGetLastError();
}

hipError_t launch_fan_step(const FanArgs& a, int round, bool last, long long nd_total, hipStream_t stream)
{
    if (a.W <= 0) return hipSuccess;
    if ((long long)a.W * a.n_h > 0x7fffffffLL || a.n_p > HMCG_FAN_MAXP) return hipErrorInvalidValue;
    const bool first = round == 1;
    hmcg::FanStepParams p{};
    p.part = a.part; p.range = a.range; p.out = a.out; p.flag = a.flag;
    p.nslab = pred_slabs(nd_total); p.nd = (double)nd_total;
    p.n_h = a.n_h; p.n_p = a.n_p; p.items_h = fan_items_h(a.n_p, first); p.rowlen = fan_max_items(a.n_h, a.n_p);
    p.first = first ? 1 : 0; p.last = last ? 1 : 0;
    for (int i = 0; i < HMCG_FAN_MAXP; ++i) p.probs[i] = i < a.n_p ? a.probs[i] : 0.0;
    hipLaunchKernelGGL(hmcg::fan_step_kernel, dim3((unsigned)(a.W * a.n_h)), dim3(hmcg::FAN_STEP_NT), 0, stream, p);
    return hipGetLastError();
}

}  // namespace hmcg_host
