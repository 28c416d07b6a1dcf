// density.hip -- chain densities and running means of a window's draws, on the device.
//
// What it replaces (joe5saia/Hmc.jl): plots/mcplots.jl:24-38 (plotchain) reads one end date's 250 000-row per-draw file back and
// draws the density of a column over the nested prefixes 1:100_000, 1:150_000, 1:200_000, 1:250_000 -- "has the chain settled";
// :47-63 (plotchainmean) draws the cumulative mean of a column over the first 10 000 draws; plots/timeseriesplots.jl:83-142
// (plot_mean / plot_var) the marginal posterior densities of every state mean and variance.  Up to the drawing these are binned
// counts, a mean and a variance per prefix and a running mean, all of one draw column; with the draws at hand in HBM they are
// one pass over that column.  The rules stand in include/hmcg.h.
//
// Shape.  The draws of a window are cut into pieces (density_plan.hpp: at every multiple of PRED_SLAB and at every cut; at most
// PRED_SLAB draws each, each inside one segment between two cuts).
//   range kernel       one block of 256 threads per (window, slab): per column the minimum and maximum of the finite x' as
//                      order-preserving 64-bit integer keys, reduced over the wave by shuffles, over the block in LDS, and
//                      folded into the window's keys by integer atomicMin / atomicMax.  Skipped when the caller gives lo_hi.
//   accumulate kernel  one block per (window, piece, column group) -- the pieces below the last cut, and beyond it those the
//                      running mean still reaches.  Thread t takes draws t, t + 256, .. of the piece; the columns are walked
//                      four at a time and the loads of such a batch stand ahead of the first rounding (a rounding between
//                      two loads makes the second wait for the first; DESIGN.md section 8 says what the ISA shows).
//                      Every column is read coalesced along d with a scalar base and a 32-bit lane offset.  The block keeps
//                      one LDS table [columns of the group][B + 3] of 32-bit counters (a piece holds at most 1024 draws),
//                      adds into it with LDS integer atomics and at the end adds the non-zero counters into the piece's
//                      SEGMENT row of the 64-bit counts in HBM with integer atomics.  S1 = sum (x' - p) and S2 = sum (x' - p)^2
//                      of the piece go through a fixed butterfly over the 64 lanes and then the four waves in wave order into
//                      the partials [window][piece][column]; p is x' of the window's draw 0.  Pieces that start inside
//                      trace_len * trace_stride also take an inclusive scan of x' - p in draw order (a shuffle scan per wave
//                      and tile, then the (tile, wave) totals in order) and leave the in-piece sums at the trace points.
//   finalize kernel    one block per (window, column): thread 0 adds the piece sums in piece order, emits mean and variance at
//                      every cut and files the sum before each piece beside the piece's own; then all threads turn the segment counts
//                      into nested prefix counts (a running sum over j) and the in-piece trace sums into running means.
//
// Deterministic: a draw's thread, tile and place in the scan depend on its place in the piece alone, the pieces on nd and the
// cuts alone; the float sums use no atomics; integer adds commute.  A launch that holds draw 0 (every device-entry call, the
// first chunk of the host entry) reads p from the data and the blocks of piece 0 file it; later chunks read it from there.
// Numerics: fp64; NaN and inf propagate into the sums of every piece that holds them and are counted in their own slots.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "density.hpp"
#include "stat_device.hpp"

namespace hmcg {

using hmcg_host::PRED_SLAB;
using hmcg_host::DENS_SLOTS;

constexpr int DN_NT = 256;                               // threads per block
constexpr int DN_NW = DN_NT / 64;
constexpr int DN_TILES = (int)(PRED_SLAB / DN_NT);       // draws per thread and column: a piece holds at most PRED_SLAB draws
constexpr int DN_CB = 4;                                 // columns per batch of loads
constexpr int DN_PART = 3;                               // per (window, piece, column): S1, S2, and the S1 of all pieces before it
static_assert(PRED_SLAB % DN_NT == 0, "a slab is a whole number of tiles");

struct DensParams {
    const double* x;
    double* part;                    // [W][np_total][C][DN_PART]
    double* piv;                     // [W][C]
    unsigned long long* kmin;        // [W][C] keys of the smallest / largest finite x'
    unsigned long long* kmax;
    double* range;                   // [W][C][2]
    unsigned long long* counts;      // [W][C][n_cuts][B + 3]
    double* stats;                   // [W][C][n_cuts][2]
    double* trace;                   // [W][C][trace_len]
    long long d_origin, n;           // x holds draws [d_origin, d_origin + n) of the run
    long long nd, nd_ld, trace_stride, trace_end;
    long long q0, nq, np_total, np_acc;      // pieces of this launch; pieces of the run; pieces below the last cut
    int64_t cuts[HMCG_MAXH];
    int W, C, B, n_cuts, trace_len, round5, gcols, ngroups;
};

// Order-preserving map of the finite doubles onto unsigned 64-bit integers (-0.0 below +0.0), and back.
__device__ __forceinline__ unsigned long long dens_key(double x)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double dens_unkey(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
constexpr unsigned long long DN_KMIN_NONE = ~0ull;       // no finite value maps here (the keys of NaNs)
constexpr unsigned long long DN_KMAX_NONE = 0ull;

__global__ __launch_bounds__(DN_NT) void density_range_kernel(const DensParams p)
{
    __shared__ unsigned long long rk[DN_NW][DN_CB][2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long nslab = (p.n + PRED_SLAB - 1) / PRED_SLAB;
    // HMCG_STAT_SLAB of stat_device.hpp with a count in place of dend (as dend - dbeg this kernel compiles to other code)
    const int w = (int)((long long)blockIdx.x / nslab);
    const long long s = (long long)blockIdx.x - (long long)w * nslab;
    const long long dbeg = s * PRED_SLAB;
    const unsigned cnt = (unsigned)(dbeg + PRED_SLAB < p.n ? PRED_SLAB : p.n - dbeg);
    const double* xw = p.x + (size_t)w * (size_t)p.C * (size_t)p.nd_ld + (size_t)dbeg;
#pragma unroll 1
    for (int cb = 0; cb < p.C; cb += DN_CB) {
        double v[DN_CB][DN_TILES];
#pragma unroll
        for (int i = 0; i < DN_CB; ++i) {
            if (cb + i < p.C) {
                const double* col = xw + (size_t)(cb + i) * (size_t)p.nd_ld;
#pragma unroll
                for (int k = 0; k < DN_TILES; ++k) {
                    const unsigned o = (unsigned)(k * DN_NT + tid);
                    v[i][k] = o < cnt ? col[o] : stat_nan();
                }
            }
        }
#pragma unroll
        for (int i = 0; i < DN_CB; ++i) {
            if (cb + i < p.C) {
                unsigned long long lo = DN_KMIN_NONE, hi = DN_KMAX_NONE;
#pragma unroll
                for (int k = 0; k < DN_TILES; ++k) {
                    const double xr = stat_in(v[i][k], p.round5);
                    if (isfinite(xr)) {
                        const unsigned long long key = dens_key(xr);
                        lo = key < lo ? key : lo;
                        hi = key > hi ? key : hi;
                    }
                }
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) {
                    const unsigned long long ol = __shfl_xor(lo, m, 64), oh = __shfl_xor(hi, m, 64);
                    lo = ol < lo ? ol : lo;
                    hi = oh > hi ? oh : hi;
                }
                if (lane == 0) { rk[wv][i][0] = lo; rk[wv][i][1] = hi; }
            }
        }
        __syncthreads();
        if (tid < DN_CB && cb + tid < p.C) {
            unsigned long long lo = rk[0][tid][0], hi = rk[0][tid][1];
#pragma unroll
            for (int q = 1; q < DN_NW; ++q) {
                lo = rk[q][tid][0] < lo ? rk[q][tid][0] : lo;
                hi = rk[q][tid][1] > hi ? rk[q][tid][1] : hi;
            }
            const size_t wc = (size_t)w * (size_t)p.C + (size_t)(cb + tid);
            if (lo != DN_KMIN_NONE) atomicMin(p.kmin + wc, lo);
            if (hi != DN_KMAX_NONE) atomicMax(p.kmax + wc, hi);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(DN_NT) void density_resolve_kernel(const DensParams p, const double* lo_hi)
{
    const long long i = (long long)blockIdx.x * DN_NT + threadIdx.x;
    if (i >= (long long)p.W * p.C) return;
    double lo, hi;
    if (lo_hi) { lo = lo_hi[2 * i]; hi = lo_hi[2 * i + 1]; }
    else {
        const unsigned long long a = p.kmin[i], b = p.kmax[i];
        const double nan = stat_nan();
        lo = a == DN_KMIN_NONE ? nan : dens_unkey(a);
        hi = a == DN_KMIN_NONE ? nan : dens_unkey(b);
    }
    p.range[2 * i] = lo;
    p.range[2 * i + 1] = hi;
}

__global__ __launch_bounds__(DN_NT) void density_accumulate_kernel(const DensParams p)
{
    extern __shared__ unsigned hist[];                   // [columns of the group][B + 3]
    __shared__ double red[DN_NW][DN_CB][2];
    __shared__ double wt[DN_TILES * DN_NW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    long long bid = (long long)blockIdx.x;
    const int g = (int)(bid % p.ngroups);
    bid /= p.ngroups;
    const long long qrel = bid % p.nq;
    const int w = (int)(bid / p.nq);
    const long long q = p.q0 + qrel;
    const hmcg_host::DensPiece pc = hmcg_host::dens_piece(q, p.nd, p.cuts, p.n_cuts);
    const unsigned cnt = (unsigned)pc.n;
    const int c0 = g * p.gcols;
    const int ncols = p.C - c0 < p.gcols ? p.C - c0 : p.gcols;
    const int nb = p.B + DENS_SLOTS;
    for (int i = tid; i < ncols * nb; i += DN_NT) hist[i] = 0u;
    __syncthreads();
    const bool tr_piece = p.trace_len > 0 && pc.d0 < p.trace_end;
    const bool own_pivot = p.d_origin == 0;
    const bool binned = pc.segment < p.n_cuts;           // a piece beyond the last cut is here for the running mean alone
    const double* x0 = p.x + ((size_t)w * (size_t)p.C + (size_t)c0) * (size_t)p.nd_ld;       // column c0 at this launch's first draw
    const double* xw = x0 + (size_t)(pc.d0 - p.d_origin);
    const double dB = (double)p.B;
#pragma unroll 1
    for (int cb = 0; cb < ncols; cb += DN_CB) {
        // every load of the batch before any rounding
        double v[DN_CB][DN_TILES], pv[DN_CB], lo[DN_CB], hi[DN_CB];
#pragma unroll
        for (int i = 0; i < DN_CB; ++i) {
            if (cb + i < ncols) {
                const double* col = xw + (size_t)(cb + i) * (size_t)p.nd_ld;
#pragma unroll
                for (int k = 0; k < DN_TILES; ++k) {
                    const unsigned o = (unsigned)(k * DN_NT + tid);
                    v[i][k] = o < cnt ? col[o] : 0.0;
                }
                const size_t wc = (size_t)w * (size_t)p.C + (size_t)(c0 + cb + i);
                pv[i] = own_pivot ? x0[(size_t)(cb + i) * (size_t)p.nd_ld] : p.piv[wc];
                lo[i] = p.range[2 * wc];
                hi[i] = p.range[2 * wc + 1];
            }
        }
#pragma unroll
        for (int i = 0; i < DN_CB; ++i) {
            if (cb + i < ncols) {
                // the pivot was rounded when it was filed; a launch that reads it from the data rounds it here (stat_in of
                // stat_device.hpp under one more condition)
                const double pvt = (own_pivot && p.round5) ? round5(pv[i]) : pv[i];
                const double width = hi[i] - lo[i];
                const double scale = dB / width;
                const bool norange = isnan(lo[i]) || isnan(hi[i]), flat = !(hi[i] > lo[i]);
                unsigned* hcol = hist + (cb + i) * nb;
                double a[DN_TILES], s1 = 0.0, s2 = 0.0;
#pragma unroll
                for (int k = 0; k < DN_TILES; ++k) {
                    const bool valid = (unsigned)(k * DN_NT + tid) < cnt;
                    const double xr = stat_in(v[i][k], p.round5);
                    if (valid && binned) {
                        int slot;
                        if (isnan(xr)) slot = p.B + 2;
                        else if (norange || xr < lo[i]) slot = p.B;
                        else if (xr > hi[i]) slot = p.B + 1;
                        else if (flat) slot = 0;
                        else {
                            const double off = xr - lo[i];
                            const double t = floor(off * scale);
                            slot = t >= dB ? p.B - 1 : (t > 0.0 ? (int)t : 0);
                        }
                        atomicAdd(hcol + slot, 1u);
                    }
                    a[k] = valid ? xr - pvt : 0.0;
                    s1 += a[k];
                    s2 = fma(a[k], a[k], s2);
                }
                HMCG_WAVE_SUM(s1);
                HMCG_WAVE_SUM(s2);
                if (lane == 0) { red[wv][i][0] = s1; red[wv][i][1] = s2; }
                if (tr_piece) {                              // block-uniform
                    double sc[DN_TILES];
#pragma unroll
                    for (int k = 0; k < DN_TILES; ++k) {
                        double t = a[k];
#pragma unroll
                        for (int m = 1; m < 64; m <<= 1) {
                            const double u = __shfl_up(t, m, 64);
                            if (lane >= m) t += u;
                        }
                        sc[k] = t;
                        if (lane == 63) wt[k * DN_NW + wv] = t;
                    }
                    __syncthreads();
                    double* tr = p.trace + ((size_t)w * (size_t)p.C + (size_t)(c0 + cb + i)) * (size_t)p.trace_len;
                    double run = 0.0;                        // the (tile, wave) totals before the current one, added in order
#pragma unroll
                    for (int k = 0; k < DN_TILES; ++k) {
#pragma unroll
                        for (int j = 0; j < DN_NW; ++j) {
                            if (j == wv) {
                                const unsigned o = (unsigned)(k * DN_NT + tid);
                                const long long e = pc.d0 + (long long)o + 1;        // draws in the prefix that ends here
                                if (o < cnt && e <= p.trace_end && e % p.trace_stride == 0) tr[e / p.trace_stride - 1] = run + sc[k];
                            }
                            run += wt[k * DN_NW + j];
                        }
                    }
                    __syncthreads();
                }
            }
        }
        __syncthreads();
        if (tid < DN_CB * 2) {
            const int i = tid >> 1, e = tid & 1;
            if (cb + i < ncols) {
                double t = red[0][i][e];
#pragma unroll
                for (int j = 1; j < DN_NW; ++j) t += red[j][i][e];
                p.part[(((size_t)w * (size_t)p.np_total + (size_t)q) * (size_t)p.C + (size_t)(c0 + cb + i)) * DN_PART + e] = t;
            }
        }
        __syncthreads();
    }
    if (own_pivot && q == 0) {
        for (int c = tid; c < ncols; c += DN_NT) {
            const double f = x0[(size_t)c * (size_t)p.nd_ld];
            p.piv[(size_t)w * (size_t)p.C + (size_t)(c0 + c)] = stat_in(f, p.round5);
        }
    }
    // the piece's counts into its segment's row; most bins of a posterior are empty
    for (int i = tid; binned && i < ncols * nb; i += DN_NT) {
        const unsigned n = hist[i];
        if (n) {
            const int c = i / nb, b = i - c * nb;
            atomicAdd(p.counts + (((size_t)w * (size_t)p.C + (size_t)(c0 + c)) * (size_t)p.n_cuts + (size_t)pc.segment) * (size_t)nb + (size_t)b,
                      (unsigned long long)n);
        }
    }
}

// One block per (window, column).
__global__ __launch_bounds__(DN_NT) void density_finalize_kernel(const DensParams p)
{
    __shared__ double ps[DN_NT][2];
    __shared__ long long qc[HMCG_MAXH];                  // pieces below cut j
    const int tid = threadIdx.x;
    const int w = (int)(blockIdx.x / (unsigned)p.C), c = (int)(blockIdx.x - (unsigned)w * (unsigned)p.C);
    const size_t wc = (size_t)w * (size_t)p.C + (size_t)c;
    const double pvt = p.piv[wc];
    if (tid < p.n_cuts) qc[tid] = hmcg_host::dens_piece_of(p.cuts[tid], p.nd, p.cuts, p.n_cuts);
    double S1 = 0.0, S2 = 0.0;
    int jc = 0;
    for (long long base = 0; base < p.np_acc; base += DN_NT) {
        __syncthreads();
        const long long q = base + tid;
        if (q < p.np_acc) {
            const double* src = p.part + (((size_t)w * (size_t)p.np_total + (size_t)q) * (size_t)p.C + (size_t)c) * DN_PART;
            ps[tid][0] = src[0];
            ps[tid][1] = src[1];
        }
        __syncthreads();
        if (tid == 0) {
            const int m = (int)(p.np_acc - base < DN_NT ? p.np_acc - base : DN_NT);
            for (int i = 0; i < m; ++i) {
                // the sum before this piece, for its trace points: beside the piece's own sums, so any number of pieces fits
                p.part[(((size_t)w * (size_t)p.np_total + (size_t)(base + i)) * (size_t)p.C + (size_t)c) * DN_PART + 2] = S1;
                S1 += ps[i][0];
                S2 += ps[i][1];
                if (jc < p.n_cuts && base + i + 1 == qc[jc]) {
                    const double n = (double)p.cuts[jc];
                    const double sq = S1 * S1;
                    const double corr = sq / n;
                    double* o = p.stats + (wc * (size_t)p.n_cuts + (size_t)jc) * 2;
                    o[0] = pvt + S1 / n;
                    o[1] = (S2 - corr) / (n - 1.0);
                    ++jc;
                }
            }
        }
    }
    __threadfence_block();                               // thread 0's sums before each piece, read by every thread below
    __syncthreads();
    const int nb = p.B + DENS_SLOTS;
    for (int b = tid; b < nb; b += DN_NT) {
        unsigned long long run = 0;
        for (int j = 0; j < p.n_cuts; ++j) {
            unsigned long long* cell = p.counts + (wc * (size_t)p.n_cuts + (size_t)j) * (size_t)nb + (size_t)b;
            run += *cell;
            *cell = run;
        }
    }
    for (int i = tid; i < p.trace_len; i += DN_NT) {
        const long long ni = (long long)(i + 1) * p.trace_stride;
        const long long q = hmcg_host::dens_piece_of(ni - 1, p.nd, p.cuts, p.n_cuts);
        double* cell = p.trace + wc * (size_t)p.trace_len + (size_t)i;
        const double before = p.part[(((size_t)w * (size_t)p.np_total + (size_t)q) * (size_t)p.C + (size_t)c) * DN_PART + 2];
        const double sum = before + *cell;
        *cell = pvt + sum / (double)ni;
    }
}

}  // namespace hmcg

namespace hmcg_host {

static size_t dens_part_doubles(int W, int C, long long np) { return (size_t)W * (size_t)np * (size_t)C * (size_t)hmcg::DN_PART; }

size_t dens_work_bytes(int W, int C, long long nd, const int64_t* cuts, int n_cuts)
{
    return sizeof(double) * (dens_part_doubles(W, C, dens_pieces(nd, cuts, n_cuts)) + (size_t)W * (size_t)C) +
           sizeof(unsigned long long) * 2 * (size_t)W * (size_t)C;
}

static bool dens_params(const DensArgs& a, hmcg::DensParams& p)
{
    if (a.C < 1 || a.C > HMCG_MAXK * HMCG_MAXK || a.B < 1 || a.B > HMCG_DENS_MAXBINS || a.n_cuts < 1 || a.n_cuts > HMCG_MAXH) return false;
    if (a.trace_len < 0 || a.trace_len > HMCG_DENS_MAXTRACE || a.trace_stride < 1) return false;
    if (a.nd < 1 || !chunk_origin_ok(a.d_origin, a.n, a.nd) || a.nd_ld < a.n) return false;
    for (int j = 0; j < a.n_cuts; ++j)
        if (a.cuts[j] < 1 || a.cuts[j] > a.nd || (j > 0 && a.cuts[j] <= a.cuts[j - 1])) return false;
    if ((long long)a.trace_len * a.trace_stride > a.nd) return false;
    p = hmcg::DensParams{};
    p.np_total = dens_pieces(a.nd, a.cuts, a.n_cuts);
    p.np_acc = dens_piece_of(a.cuts[a.n_cuts - 1], a.nd, a.cuts, a.n_cuts);
    if (a.trace_len > 0) {                               // the running mean may reach beyond the last cut
        const long long qt = dens_piece_of((long long)a.trace_len * a.trace_stride - 1, a.nd, a.cuts, a.n_cuts) + 1;
        if (qt > p.np_acc) p.np_acc = qt;
    }
    p.x = a.x;
    p.part = reinterpret_cast<double*>(a.work);
    p.piv = p.part + dens_part_doubles(a.W, a.C, p.np_total);
    p.kmin = reinterpret_cast<unsigned long long*>(p.piv + (size_t)a.W * (size_t)a.C);
    p.kmax = p.kmin + (size_t)a.W * (size_t)a.C;
    p.range = a.range; p.counts = a.counts; p.stats = a.stats; p.trace = a.trace;
    p.d_origin = a.d_origin; p.n = a.n; p.nd = a.nd; p.nd_ld = a.nd_ld;
    p.trace_stride = a.trace_stride; p.trace_end = (long long)a.trace_len * a.trace_stride;
    for (int j = 0; j < HMCG_MAXH; ++j) p.cuts[j] = j < a.n_cuts ? a.cuts[j] : 0;
    p.W = a.W; p.C = a.C; p.B = a.B; p.n_cuts = a.n_cuts; p.trace_len = a.trace_len; p.round5 = a.round5 ? 1 : 0;
    p.gcols = dens_group_cols(a.C, a.B); p.ngroups = dens_groups(a.C, a.B);
    const long long q0 = dens_piece_of(a.d_origin, a.nd, a.cuts, a.n_cuts);
    long long q1 = dens_piece_of(a.d_origin + a.n, a.nd, a.cuts, a.n_cuts);
    if (q1 > p.np_acc) q1 = p.np_acc;
    p.q0 = q0; p.nq = q1 > q0 ? q1 - q0 : 0;
    return true;
}

hipError_t launch_density_clear(const DensArgs& a, hipStream_t stream)
{
    if (a.W <= 0) return hipSuccess;
    hmcg::DensParams p;
    if (!dens_params(a, p)) return hipErrorInvalidValue;
    const size_t wc = (size_t)a.W * (size_t)a.C;
    hipError_t e = hipMemsetAsync(p.kmin, 0xff, sizeof(unsigned long long) * wc, stream);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(p.kmax, 0, sizeof(unsigned long long) * wc, stream);
    if (e != hipSuccess) return e;
    return hipMemsetAsync(a.counts, 0, sizeof(unsigned long long) * wc * (size_t)a.n_cuts * (size_t)(a.B + DENS_SLOTS), stream);
}

hipError_t launch_density_range(const DensArgs& a, hipStream_t stream)
{
    if (a.W <= 0) return hipSuccess;
    hmcg::DensParams p;
    if (!dens_params(a, p)) return hipErrorInvalidValue;
    const long long blocks = (long long)a.W * pred_slabs(a.n);
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hmcg::density_range_kernel, dim3((unsigned)blocks), dim3(hmcg::DN_NT), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_density_resolve(const DensArgs& a, const double* lo_hi, hipStream_t stream)
{
    if (a.W <= 0) return hipSuccess;
    hmcg::DensParams p;
    if (!dens_params(a, p)) return hipErrorInvalidValue;
    const long long n = (long long)a.W * a.C;
    hipLaunchKernelGGL(hmcg::density_resolve_kernel, dim3((unsigned)((n + hmcg::DN_NT - 1) / hmcg::DN_NT)), dim3(hmcg::DN_NT), 0, stream, p, lo_hi);
    return hipGetLastError();
}

hipError_t launch_density_accumulate(const DensArgs& a, hipStream_t stream)
{
    if (a.W <= 0) return hipSuccess;
    hmcg::DensParams p;
    if (!dens_params(a, p)) return hipErrorInvalidValue;
    if (p.nq == 0) return hipSuccess;                    // every draw of this block lies beyond the last cut
    const long long blocks = (long long)a.W * p.nq * p.ngroups;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const size_t lds = sizeof(unsigned) * (size_t)p.gcols * (size_t)(a.B + DENS_SLOTS);
    hipLaunchKernelGGL(hmcg::density_accumulate_kernel, dim3((unsigned)blocks), dim3(hmcg::DN_NT), lds, stream, p);
    return hipGetLastError();
}

hipError_t launch_density_finalize(const DensArgs& a, hipStream_t stream)
{
    if (a.W <= 0) return hipSuccess;
    hmcg::DensParams p;
    if (!dens_params(a, p)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hmcg::density_finalize_kernel, dim3((unsigned)((long long)a.W * a.C)), dim3(hmcg::DN_NT), 0, stream, p);
    return hipGetLastError();
}

}  // namespace hmcg_host
