// score.hip -- proper scores of the predictive regime mixture against the realised value, per window and horizon, on the
// device: the continuous ranked probability score CRPS(F, y) = E|X - y| - 0.5 E|X - X'|, the probability integral transform
// F(y) and the density F'(y).
//
// What it adds: the reference verifies a forecast by the point forecast's error alone.  F is the mixture of N = n_u * K normals
// whose CDF predictive.hip evaluates, so E|X - X'| is a sum over all N^2 component pairs of the closed form a(m, S2) = E|N(m, S2)|
// (include/hmcg_score.h states every expression and order; score_plan.hpp holds a() and the cut of the square).  The pair value
// does not depend on the horizon -- only the weights do -- so one pass over the pairs serves every horizon.
//
// score_comp_kernel has the tile shape of predictive_cdf_kernel: one block per (window, slab of PRED_SLAB used draws), a tile of
// 64 draws staged in LDS with the weights of every horizon (the transition staging and the weights of mixture_tile.hpp).  It
// writes the used draws' components (mu, sig2, rounded if asked) and weights into the work area, and a thread per (draw,
// horizon) evaluates F, E|.| and the density at that
// horizon's realised value with predictive.hip's per-draw expression; one thread per (value, horizon) adds them in draw order.
// score_pair_kernel, the hot path: a block owns two rows of tiles of the component square (a short and a long one: equal work),
// thread t one component of each row; the column tiles (mu, sig2, the n_h weights of a component, side by side) are staged in
// LDS and read as broadcasts -- every lane the same address, no bank conflict -- and a() is evaluated once per pair for n_h
// accumulators.  Only tiles on or below the diagonal are visited; those below count twice.
// score_finish_kernel: a thread per (window, horizon) adds slab sums and block partials in order and forms the five outputs.
// Deterministic: no atomics anywhere.  fp64 throughout, no scratch, no inline assembly.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "score.hpp"
#include "mixture_tile.hpp"

namespace hmcg {

using hmcg_host::SCORE_TP;

constexpr int SCORE_FIN_NT = 64;

struct ScoreCompParams {
    const double* mu; const double* sig2; const double* pi_end; const double* A; const double* yreal;
    double* work;
    long long n_u, stride, nd_ld, nslab, yreal_ld, w0;
    hmcg_host::ScoreWork lay;
    int n_h, round5;
    int hz[HMCG_MAXH];
};

template <int K>
__global__ __launch_bounds__(MIXTILE_NT) void score_comp_kernel(const ScoreCompParams p)
{
    extern __shared__ double score_lds[];
    const int n_h = p.n_h;
    double* MC = score_lds;                              // [MIXTILE_TD][K][3]: mu, sig2, c
    double* Ws = MC + MIXTILE_TD * K * 3;                // [MIXTILE_TD][n_h][K]: weights of every horizon
    double* Vs = Ws + MIXTILE_TD * n_h * K;              // [3][n_h][MIXTILE_TD]: F, E, P of a (draw, horizon)
    double* Ys = Vs + 3 * n_h * MIXTILE_TD;              // [HMCG_MAXH]: the window's realised values
    double* As = Ys + HMCG_MAXH;                         // [K * K][MIXTILE_TD]: transition draws (present with a horizon > 0)
    const int tid = threadIdx.x;
    HMCG_STAT_SLAB(w, s, ubeg, uend, p.nslab, p.n_u);
    const double* mu = p.mu + (size_t)w * K * p.nd_ld;
    const double* sig2 = p.sig2 + (size_t)w * K * p.nd_ld;
    const double* pie = p.pi_end + (size_t)w * K * p.nd_ld;
    const double* At = p.A ? p.A + (size_t)w * K * K * p.nd_ld : nullptr;
    double* wk = p.work + (size_t)w * p.lay.total;
    const size_t N = (size_t)p.n_u * K;
    if (tid < n_h) Ys[tid] = p.yreal[(size_t)tid * (size_t)p.yreal_ld + (size_t)(p.w0 + w)];
    double acc = 0.0;
#define SCORE_DRAW(dd) (size_t)(u0 + (dd)) * (size_t)p.stride
    for (long long u0 = ubeg; u0 < uend; u0 += MIXTILE_TD) {
        const int nv = uend - u0 < MIXTILE_TD ? (int)(uend - u0) : MIXTILE_TD;
        // HMCG_MIX_STAGE_MC of mixture_tile.hpp, three wide and with the work area's copy; neither kernel takes the other's form
        for (int q = tid; q < K * MIXTILE_TD; q += MIXTILE_NT) {
            const int k = q / MIXTILE_TD, dd = q - k * MIXTILE_TD;
            if (dd < nv) {
                const size_t off = (size_t)k * p.nd_ld + SCORE_DRAW(dd);
                const double m = stat_in(mu[off], p.round5), v = stat_in(sig2[off], p.round5);
                MC[(dd * K + k) * 3] = m;
                MC[(dd * K + k) * 3 + 1] = v;
                MC[(dd * K + k) * 3 + 2] = 1.0 / (1.4142135623730951 * sqrt(v));
                const size_t c = (size_t)(u0 + dd) * K + k;
                wk[p.lay.o_mu + c] = m;
                wk[p.lay.o_v + c] = v;
            }
        }
        HMCG_MIX_STAGE_A(K, As, At, p, SCORE_DRAW, nv, tid);
        __syncthreads();
        HMCG_MIX_WEIGHTS(K, Ws, As, pie, p, SCORE_DRAW, nv, n_h, tid, wk[p.lay.o_w + (size_t)jh_ * N + (size_t)(u0 + dd_) * K + k_] = wv_[k_]);
        __syncthreads();
        for (int q = tid; q < n_h * MIXTILE_TD; q += MIXTILE_NT) {
            const int jh = q / MIXTILE_TD, dd = q - jh * MIXTILE_TD;
            if (dd >= nv) continue;
            const double y = Ys[jh];
            const double* mc = MC + dd * K * 3;
            const double* wj = Ws + (dd * n_h + jh) * K;
            double F = 0.0, E = 0.0, P = 0.0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                double ph, ak, dk;
                hmcg_host::score_point(y, mc[3 * k], mc[3 * k + 1], mc[3 * k + 2], &ph, &ak, &dk);
                F = k == 0 ? wj[0] * ph : fma(wj[k], ph, F);
                E = k == 0 ? wj[0] * ak : fma(wj[k], ak, E);
                P = k == 0 ? wj[0] * dk : fma(wj[k], dk, P);
            }
            Vs[jh * MIXTILE_TD + dd] = F;
            Vs[(n_h + jh) * MIXTILE_TD + dd] = E;
            Vs[(2 * n_h + jh) * MIXTILE_TD + dd] = P;
        }
        __syncthreads();
        if (tid < 3 * n_h) {
            const double* v = Vs + tid * MIXTILE_TD;
#pragma unroll 1
            for (int dd = 0; dd < nv; ++dd) acc += v[dd];
        }
    }
#undef SCORE_DRAW
    if (tid < 3 * n_h) wk[p.lay.o_lin + (size_t)s * (size_t)(3 * n_h) + (size_t)tid] = acc;
}

struct ScorePairParams {
    double* work;
    long long N, nT, nblk;
    hmcg_host::ScoreWork lay;
};

template <int NH>
__global__ __launch_bounds__(SCORE_TP) void score_pair_kernel(const ScorePairParams p)
{
    constexpr int S = 2 + NH;                            // doubles of a staged component: mu, sig2, the NH weights
    __shared__ double Tc[SCORE_TP * S];
    __shared__ double Rw[SCORE_TP / 64][NH];
    const int tid = threadIdx.x;
    const int w = (int)((long long)blockIdx.x / p.nblk);
    const long long b = (long long)blockIdx.x - (long long)w * p.nblk;
    double* wk = p.work + (size_t)w * p.lay.total;
    const double* M = wk + p.lay.o_mu;
    const double* V = wk + p.lay.o_v;
    const double* Wt = wk + p.lay.o_w;
    const size_t N = (size_t)p.N;
    double off[NH], diag[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) { off[h] = 0.0; diag[h] = 0.0; }
    long long rows[2];
    const int nrows = hmcg_host::score_rows(p.nT, b, rows);
    for (int rr = 0; rr < nrows; ++rr) {
        const long long r = rows[rr];
        const size_t i = (size_t)r * SCORE_TP + (size_t)tid;
        const bool live = i < N;
        double mi = 0.0, vi = 0.0, wi[NH];
        if (live) { mi = M[i]; vi = V[i]; }
#pragma unroll
        for (int h = 0; h < NH; ++h) wi[h] = live ? Wt[(size_t)h * N + i] : 0.0;
        for (long long J = 0; J <= r; ++J) {
            const size_t c0 = (size_t)J * SCORE_TP;
            const int nv = N - c0 < (size_t)SCORE_TP ? (int)(N - c0) : SCORE_TP;
            __syncthreads();
            if (tid < nv) {
                Tc[tid * S] = M[c0 + tid];
                Tc[tid * S + 1] = V[c0 + tid];
#pragma unroll
                for (int h = 0; h < NH; ++h) Tc[tid * S + 2 + h] = Wt[(size_t)h * N + c0 + tid];
            }
            __syncthreads();
            if (!live) continue;
            // the last tile of a row is the diagonal one: its terms go to diag, every other tile's to off
            const bool on_diag = J == r;
            if (on_diag) {
#pragma unroll
                for (int h = 0; h < NH; ++h) { const double t = off[h]; off[h] = diag[h]; diag[h] = t; }
            }
#pragma unroll 2
            for (int j = 0; j < nv; ++j) {
                const double* cj = Tc + j * S;
                const double a = hmcg_host::score_a(mi - cj[0], vi + cj[1]);
#pragma unroll
                for (int h = 0; h < NH; ++h) {
#pragma clang fp contract(off)
                    const double ww = wi[h] * cj[2 + h];
                    const double term = ww * a;
                    off[h] = off[h] + term;
                }
            }
            if (on_diag) {
#pragma unroll
                for (int h = 0; h < NH; ++h) { const double t = off[h]; off[h] = diag[h]; diag[h] = t; }
            }
        }
    }
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        double v = (off[h] + off[h]) + diag[h];
        HMCG_WAVE_SUM(v);
        if ((tid & 63) == 0) Rw[tid >> 6][h] = v;
    }
    __syncthreads();
    if (tid < NH) {
        double sum = Rw[0][tid];
#pragma unroll
        for (int q = 1; q < SCORE_TP / 64; ++q) sum += Rw[q][tid];
        wk[p.lay.o_pair + (size_t)b * NH + (size_t)tid] = sum;
    }
}

struct ScoreFinishParams {
    const double* work;
    double* out;
    long long nslab, nblk;
    hmcg_host::ScoreWork lay;
    double n_u;
    int W, n_h;
};

__global__ __launch_bounds__(SCORE_FIN_NT) void score_finish_kernel(const ScoreFinishParams p)
{
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * SCORE_FIN_NT + threadIdx.x;
    if (e >= (long long)p.W * p.n_h) return;
    const int w = (int)(e / p.n_h), j = (int)(e - (long long)w * p.n_h);
    const double* wk = p.work + (size_t)w * p.lay.total;
    const double* lin = wk + p.lay.o_lin;
    const int rl = 3 * p.n_h;
    HMCG_SLAB_SUM(sF, lin + j, p.nslab, rl);
    HMCG_SLAB_SUM(sE, lin + p.n_h + j, p.nslab, rl);
    HMCG_SLAB_SUM(sP, lin + 2 * p.n_h + j, p.nslab, rl);
    HMCG_SLAB_SUM(sA, wk + p.lay.o_pair + j, p.nblk, p.n_h);
    const double nn = p.n_u * p.n_u;
    const double e_abs = sE / p.n_u, e_pair = sA / nn;
    const double half = 0.5 * e_pair;
    double* o = p.out + HMCG_SCORE_STRIDE * (size_t)e;
    o[0] = e_abs - half;
    o[1] = e_abs;
    o[2] = e_pair;
    o[3] = sF / p.n_u;
    o[4] = sP / p.n_u;
}

}  // namespace hmcg

namespace hmcg_host {

size_t score_lds_bytes(int K, int n_h, bool with_A)
{
    return sizeof(double) * ((size_t)hmcg::MIXTILE_TD * (size_t)(3 * K + n_h * K + 3 * n_h + (with_A ? K * K : 0)) + HMCG_MAXH);
}

// What every launch needs to hold: the strided reads stay inside the arrays, the grids inside one launch.
static bool score_args_ok(const ScoreArgs& a)
{
    if (a.W < 1 || a.n_u < 1 || a.stride < 1 || a.K < 2 || a.K > HMCG_MAXK || a.n_h < 1 || a.n_h > HMCG_MAXH) return false;
    if ((a.n_u - 1) > (a.nd_ld - 1) / a.stride) return false;           // (n_u - 1) * stride < nd_ld, without overflow
    if (a.w0 < 0 || a.w0 + a.W > a.yreal_ld) return false;
    const long long nblk = score_blocks(score_comps(a.n_u, a.K)), nslab = pred_slabs(a.n_u);
    return (long long)a.W * nblk <= 0x7fffffffLL && (long long)a.W * nslab <= 0x7fffffffLL && (long long)a.W * a.n_h <= 0x7fffffffLL;
}

hipError_t launch_score_components(const ScoreArgs& a, hipStream_t stream)
{
    if (!score_args_ok(a)) return hipErrorInvalidValue;
    hmcg::ScoreCompParams p{};
    p.mu = a.mu; p.sig2 = a.sig2; p.pi_end = a.pi_end; p.A = a.A; p.yreal = a.yreal; p.work = a.work;
    p.n_u = a.n_u; p.stride = a.stride; p.nd_ld = a.nd_ld; p.nslab = pred_slabs(a.n_u); p.yreal_ld = a.yreal_ld; p.w0 = a.w0;
    p.lay = score_work(a.n_u, a.K, a.n_h);
    p.n_h = a.n_h; p.round5 = a.round5 ? 1 : 0;
    const bool with_A = fill_horizons(a.n_h, a.horizons, p.hz);
    if (with_A && !a.A) return hipErrorInvalidValue;
    if (!with_A) p.A = nullptr;
    const size_t lds = score_lds_bytes(a.K, a.n_h, with_A);
    const dim3 grid((unsigned)((long long)a.W * p.nslab)), block(hmcg::MIXTILE_NT);
#define HMCG_SCORE_COMP(K_) HMCG_LAUNCH_LDS(hmcg::score_comp_kernel<K_>, grid, block, lds, stream, p)
    HMCG_SWITCH_K(a.K, HMCG_SCORE_COMP)
#undef HMCG_SCORE_COMP
    return hipGetLastError();
}

hipError_t launch_score_pairs(const ScoreArgs& a, hipStream_t stream)
{
    if (!score_args_ok(a)) return hipErrorInvalidValue;
    hmcg::ScorePairParams p{};
    p.work = a.work;
    p.N = score_comps(a.n_u, a.K); p.nT = score_tiles(p.N); p.nblk = score_blocks(p.N);
    p.lay = score_work(a.n_u, a.K, a.n_h);
    const dim3 grid((unsigned)((long long)a.W * p.nblk)), block(SCORE_TP);
#define HMCG_SCORE_PAIR(NH_) hipLaunchKernelGGL(hmcg::score_pair_kernel<NH_>, grid, block, 0, stream, p)
    static_assert(HMCG_MAXH == 8, "the switch lists the cases");
    switch (a.n_h) {
        case 1: HMCG_SCORE_PAIR(1); break;
        case 2: HMCG_SCORE_PAIR(2); break;
        case 3: HMCG_SCORE_PAIR(3); break;
        case 4: HMCG_SCORE_PAIR(4); break;
        case 5: HMCG_SCORE_PAIR(5); break;
        case 6: HMCG_SCORE_PAIR(6); break;
        case 7: HMCG_SCORE_PAIR(7); break;
        case 8: HMCG_SCORE_PAIR(8); break;
        default: return hipErrorInvalidValue;
    }
#undef HMCG_SCORE_PAIR
    return hipGetLastError();
}

hipError_t launch_score_finish(const ScoreArgs& a, hipStream_t stream)
{
    if (!score_args_ok(a)) return hipErrorInvalidValue;
    hmcg::ScoreFinishParams p{};
    p.work = a.work; p.out = a.out;
    p.nslab = pred_slabs(a.n_u); p.nblk = score_blocks(score_comps(a.n_u, a.K));
    p.lay = score_work(a.n_u, a.K, a.n_h);
    p.n_u = (double)a.n_u; p.W = a.W; p.n_h = a.n_h;
    const long long items = (long long)a.W * a.n_h;
    hipLaunchKernelGGL(hmcg::score_finish_kernel, dim3((unsigned)((items + hmcg::SCORE_FIN_NT - 1) / hmcg::SCORE_FIN_NT)), dim3(hmcg::SCORE_FIN_NT), 0,
                       stream, p);
    return hipGetLastError();
}

}  // namespace hmcg_host
