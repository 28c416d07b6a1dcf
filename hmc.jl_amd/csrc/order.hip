// order.hip -- exact quantiles and credible limits of a window's draws, on the device: a selection, not a sum.
//
// What it replaces: every report of a fit starts with the median and a credible interval of each parameter and forecast; to
// take them exactly a caller had to pull every draw column over PCIe and sort it (hmc.chainquantiles reads them off
// hmcg_chain_density's bins, at bin resolution).  The rules stand in include/hmcg_order.h.
//
// Shape.  One block of 1024 threads per (window, column); nothing is shared between blocks and no work memory is needed.
//   The value x' of a draw becomes its order-preserving 64-bit key (order_plan.hpp).  Every probability asks for two ranks,
//   j and min(j + 1, m - 1): up to 32 TARGETS per column, carried together and kept sorted by rank, so that the key prefixes
//   they have reached stand in ascending order and targets with one prefix share one set of counters.
//   pass 0          counts the NaNs (m = nd - nan fixes the ranks) and histograms the top digit of every key.
//   digit pass d    histograms digit d of the keys whose higher digits equal one of the distinct prefixes (a binary search
//                   over at most 32 prefixes in LDS); [distinct prefixes][256] 32-bit LDS counters, 32 KB at most.
//   resolve         after every pass each row of counters becomes its running sum (one wave per row); a target finds its
//                   digit by bisection, keeps its rank inside that bucket, and thread 0 rebuilds the distinct prefixes.
//   candidate pass  as soon as the buckets of all distinct prefixes together hold at most ORD_CAP keys, one more pass gathers
//                   them into the same LDS buffer, a bitonic sort orders them and every target reads its key off the sorted
//                   list (buckets stand in prefix order; a target is at its bucket's start + its rank in the bucket).
//   A bucket that never shrinks -- ties, as in a pi_end column that is mostly exactly 1 -- is carried to the last digit, where
//   the prefix IS the key.  A column is read at most ORD_DIGITS = 8 times: d digit passes and the candidate pass, d <= 7, or 8
//   digit passes.  Posterior draws narrow in the second and third digit: four reads as a rule.
//   A thread keeps the counter it hit last and how often, and adds when the next key hits another one: runs of ties cost one
//   LDS atomic, not one each.  The loads of a tile of four draws per thread stand ahead of the first rounding.
//
// Deterministic: integer counters only (LDS atomics commute); the candidates arrive in any order and are sorted; lo and hi are
// the keys mapped back, bit copies of x'.  No floating-point accumulation anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "order.hpp"
#include "stat_device.hpp"

namespace hmcg {

using hmcg_host::ORD_BITS;
using hmcg_host::ORD_CAP;
using hmcg_host::ORD_DIGITS;
using hmcg_host::ORD_MASK;
using hmcg_host::ORD_MAXT;

constexpr int OQ_NT = 1024;                              // threads per block
constexpr int OQ_NW = OQ_NT / 64;
constexpr int OQ_U = 4;                                  // draws per thread and tile
constexpr int OQ_BINS = 1 << ORD_BITS;
constexpr unsigned OQ_NONE = 0xffffffffu;                // no counter: a NaN, the padding of a tile, a key off every prefix
constexpr unsigned long long OQ_PAD = ~0ull;             // above every prefix and every key of a non-NaN value

struct OrdParams {
    const double* x;
    double* q;
    long long* n;
    long long nd, ld;
    int Q, round5;
    double probs[HMCG_ORD_MAXQ];
};

// A draw as the selection ranks it: stat_in of stat_device.hpp, and a zero keeps the sign of the draw (a quotient -0.0 / 1e5 is
// -0.0; the other statistics never see the sign of a zero, the total order does).
__device__ __forceinline__ double ord_in(double x, int r5)
{
    const double q = stat_in(x, r5);
    return q == 0.0 ? copysign(0.0, x) : q;
}
__device__ __forceinline__ unsigned long long ord_dkey(double x) { return hmcg_host::ord_key_of_bits((unsigned long long)__double_as_longlong(x)); }
__device__ __forceinline__ double ord_dunkey(unsigned long long k) { return __longlong_as_double((long long)hmcg_host::ord_bits_of_key(k)); }

// Index of prefix kp among the ascending distinct prefixes (padded with OQ_PAD to ORD_MAXT), or OQ_NONE.  top: the largest
// power of two <= P - 1 (0 for one prefix).
__device__ __forceinline__ unsigned ord_slot(const unsigned long long* dpre, unsigned top, unsigned long long kp)
{
    unsigned lo = 0;
    for (unsigned st = top; st; st >>= 1)
        if (dpre[lo + st] <= kp) lo += st;
    return dpre[lo] == kp ? lo : OQ_NONE;
}

// One more hit of counter id_ (OQ_NONE: none): the run of the counter hit last is added when another one is hit.
#define OQ_HIT(hist_, cur_, run_, id_)                                                                                    \
    do {                                                                                                                  \
        if ((id_) != cur_) {                                                                                              \
            if (cur_ != OQ_NONE) atomicAdd((hist_) + cur_, run_);                                                         \
            cur_ = (id_);                                                                                                 \
            run_ = 0u;                                                                                                    \
        }                                                                                                                 \
        ++run_;                                                                                                           \
    } while (0)

// A tile of the column: OQ_U draws per thread, every load ahead of the first rounding.  Declares v_[OQ_U]; draw k_ of the
// tile is valid when OQ_VALID(base_, k_).
#define OQ_VALID(base_, k_) ((base_) + (long long)((k_) * OQ_NT + tid) < p.nd)
#define OQ_LOAD_TILE(v_, base_)                                                                                           \
    double v_[OQ_U];                                                                                                      \
    _Pragma("unroll") for (int k_ = 0; k_ < OQ_U; ++k_)                                                                   \
        v_[k_] = OQ_VALID(base_, k_) ? col[(size_t)(base_) + (size_t)(k_ * OQ_NT + tid)] : 0.0

__global__ __launch_bounds__(OQ_NT) void chain_quantiles_kernel(const OrdParams p)
{
    __shared__ unsigned long long buf[ORD_CAP];          // [distinct prefixes][OQ_BINS] 32-bit counters | the candidate keys
    __shared__ unsigned long long dpre[ORD_MAXT];        // distinct prefixes, ascending, padded with OQ_PAD
    __shared__ unsigned long long tkey[ORD_MAXT];        // target t (in rank order): its prefix so far; at the end its key
    __shared__ unsigned trank[ORD_MAXT];                 // its rank inside its bucket
    __shared__ unsigned tslot[ORD_MAXT];                 // its distinct prefix
    __shared__ unsigned tcnt[ORD_MAXT];                  // keys in its bucket
    __shared__ unsigned tpos[ORD_MAXT];                  // target 2 i + e of probability i -> its place in rank order
    __shared__ unsigned dbase[ORD_MAXT];                 // keys in the buckets of the distinct prefixes below this one
    __shared__ double sprob[HMCG_ORD_MAXQ];
    __shared__ unsigned s_nan, s_P, s_gather, s_ncand;
    unsigned* hist = reinterpret_cast<unsigned*>(buf);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int T = 2 * p.Q;
    const double* col = p.x + (size_t)blockIdx.x * (size_t)p.ld;
    double* qo = p.q + (size_t)blockIdx.x * (size_t)p.Q * HMCG_ORD_STRIDE;
    long long* no = p.n + (size_t)blockIdx.x * 2;

    if (tid < OQ_BINS) hist[tid] = 0u;
    if (tid < HMCG_ORD_MAXQ) {
        double pr = 0.0;
#pragma unroll
        for (int i = 0; i < HMCG_ORD_MAXQ; ++i) pr = tid == i ? p.probs[i] : pr;
        sprob[tid] = pr;
    }
    if (tid == 0) { s_nan = 0u; dpre[0] = 0ull; }
    if (tid < ORD_MAXT) tslot[tid] = 0u;
    __syncthreads();

    // pass 0: the NaNs and the top digit of every key
    {
        unsigned cur = OQ_NONE, run = 0u, nn = 0u;
#pragma unroll 1
        for (long long base = 0; base < p.nd; base += OQ_NT * OQ_U) {
            OQ_LOAD_TILE(v, base);
#pragma unroll
            for (int k = 0; k < OQ_U; ++k) {
                const double xr = ord_in(v[k], p.round5);
                const bool valid = OQ_VALID(base, k), isn = isnan(xr);
                nn += valid && isn ? 1u : 0u;
                const unsigned id = valid && !isn ? (unsigned)(ord_dkey(xr) >> hmcg_host::ord_shift(0)) : OQ_NONE;
                OQ_HIT(hist, cur, run, id);
            }
        }
        if (cur != OQ_NONE) atomicAdd(hist + cur, run);
        if (nn) atomicAdd(&s_nan, nn);
    }
    __syncthreads();
    const unsigned nan = s_nan;
    const long long m = p.nd - (long long)nan;
    if (tid == 0) { no[0] = m; no[1] = (long long)nan; }
    if (m == 0) {                                            // block-uniform
        if (tid < p.Q * HMCG_ORD_STRIDE) qo[tid] = stat_nan();
        return;
    }
    // the targets' ranks in the column, and their rank order (ties by target number)
    if (tid < T) {
        const hmcg_host::OrdRank r = hmcg_host::ord_rank(sprob[tid >> 1], m);
        const long long up = r.j + 1 < m - 1 ? r.j + 1 : m - 1;
        tcnt[tid] = (unsigned)((tid & 1) ? up : r.j);
    }
    __syncthreads();
    if (tid < T) {
        const unsigned r = tcnt[tid];
        unsigned pos = 0u;
        for (int u = 0; u < T; ++u) {
            const unsigned ru = tcnt[u];
            pos += (ru < r || (ru == r && u < tid)) ? 1u : 0u;
        }
        tpos[tid] = pos;
        trank[pos] = r;
    }
    __syncthreads();

    int d = 0;                                               // the digit the counters in `hist` are of
    for (;;) {
        // resolve: every row of counters to its running sum ...
        const int P = d == 0 ? 1 : (int)s_P;
        for (int s = wv; s < P; s += OQ_NW) {
            unsigned* row = hist + s * OQ_BINS;
            const unsigned a0 = row[4 * lane], a1 = row[4 * lane + 1], a2 = row[4 * lane + 2], a3 = row[4 * lane + 3];
            const unsigned own = a0 + a1 + a2 + a3;
            unsigned t = own;
#pragma unroll
            for (int mm = 1; mm < 64; mm <<= 1) {
                const unsigned u = __shfl_up(t, mm, 64);
                if (lane >= mm) t += u;
            }
            const unsigned ex = t - own;
            row[4 * lane] = ex + a0;
            row[4 * lane + 1] = ex + a0 + a1;
            row[4 * lane + 2] = ex + a0 + a1 + a2;
            row[4 * lane + 3] = t;
        }
        __syncthreads();
        // ... a target's digit is the first whose running sum exceeds its rank
        if (tid < T) {
            const unsigned s = tslot[tid], r = trank[tid];
            const unsigned* row = hist + s * OQ_BINS;
            unsigned b = 0u;
#pragma unroll
            for (unsigned st = OQ_BINS / 2; st; st >>= 1)
                if (row[b + st - 1u] <= r) b += st;
            const unsigned below = b ? row[b - 1u] : 0u;
            trank[tid] = r - below;
            tcnt[tid] = row[b] - below;
            tkey[tid] = (d == 0 ? 0ull : dpre[s] << ORD_BITS) | (unsigned long long)b;
        }
        __syncthreads();
        if (tid == 0) {
            unsigned np = 0u;
            unsigned long long total = 0ull;
            for (int t = 0; t < T; ++t) {
                if (t == 0 || tkey[t] != tkey[t - 1]) {
                    dpre[np] = tkey[t];
                    dbase[np] = (unsigned)total;
                    total += tcnt[t];
                    ++np;
                }
                tslot[t] = np - 1u;
            }
            for (int t = (int)np; t < ORD_MAXT; ++t) dpre[t] = OQ_PAD;
            s_P = np;
            s_gather = total <= (unsigned long long)ORD_CAP ? 1u : 0u;
            s_ncand = 0u;
        }
        __syncthreads();
        ++d;
        if (d == ORD_DIGITS) break;                          // every digit consumed: tkey is the key
        const int np = (int)s_P;
        const unsigned top = np <= 1 ? 0u : 1u << (31 - __clz(np - 1));
        const int shift = hmcg_host::ord_shift(d), pshift = shift + ORD_BITS;
        if (s_gather) {
            // candidate pass: the keys of every distinct prefix's bucket into LDS, sorted there
#pragma unroll 1
            for (long long base = 0; base < p.nd; base += OQ_NT * OQ_U) {
                OQ_LOAD_TILE(v, base);
#pragma unroll
                for (int k = 0; k < OQ_U; ++k) {
                    const double xr = ord_in(v[k], p.round5);
                    if (OQ_VALID(base, k) && !isnan(xr)) {
                        const unsigned long long key = ord_dkey(xr);
                        if (ord_slot(dpre, top, key >> pshift) != OQ_NONE) {
                            const unsigned at = atomicAdd(&s_ncand, 1u);
                            if (at < (unsigned)ORD_CAP) buf[at] = key;
                        }
                    }
                }
            }
            __syncthreads();
            const unsigned nc = s_ncand < (unsigned)ORD_CAP ? s_ncand : (unsigned)ORD_CAP;
            unsigned n2 = 2u;
            while (n2 < nc) n2 <<= 1;
            for (unsigned i = nc + tid; i < n2; i += OQ_NT) buf[i] = OQ_PAD;
            __syncthreads();
            for (unsigned k = 2u; k <= n2; k <<= 1) {
                for (unsigned j = k >> 1; j; j >>= 1) {
                    for (unsigned i = tid; i < n2; i += OQ_NT) {
                        const unsigned l = i ^ j;
                        if (l > i) {
                            const unsigned long long a = buf[i], b = buf[l];
                            if ((a > b) == ((i & k) == 0u)) { buf[i] = b; buf[l] = a; }
                        }
                    }
                    __syncthreads();
                }
            }
            if (tid < T) {
                unsigned at = dbase[tslot[tid]] + trank[tid];
                at = at < n2 ? at : n2 - 1u;
                tkey[tid] = buf[at];
            }
            __syncthreads();
            break;
        }
        // digit pass d
        for (int i = tid; i < np * OQ_BINS; i += OQ_NT) hist[i] = 0u;
        __syncthreads();
        {
            unsigned cur = OQ_NONE, run = 0u;
#pragma unroll 1
            for (long long base = 0; base < p.nd; base += OQ_NT * OQ_U) {
                OQ_LOAD_TILE(v, base);
#pragma unroll
                for (int k = 0; k < OQ_U; ++k) {
                    const double xr = ord_in(v[k], p.round5);
                    unsigned id = OQ_NONE;
                    if (OQ_VALID(base, k) && !isnan(xr)) {
                        const unsigned long long key = ord_dkey(xr);
                        const unsigned s = ord_slot(dpre, top, key >> pshift);
                        if (s != OQ_NONE) id = s * OQ_BINS + ((unsigned)(key >> shift) & ORD_MASK);
                    }
                    OQ_HIT(hist, cur, run, id);
                }
            }
            if (cur != OQ_NONE) atomicAdd(hist + cur, run);
        }
        __syncthreads();
    }

    if (tid < p.Q) {
        const double lo = ord_dunkey(tkey[tpos[2 * tid]]), hi = ord_dunkey(tkey[tpos[2 * tid + 1]]);
        const double g = hmcg_host::ord_rank(sprob[tid], m).g;
        double* o = qo + (size_t)tid * HMCG_ORD_STRIDE;
        o[0] = hmcg_host::ord_value(lo, hi, g);
        o[1] = lo;
        o[2] = hi;
        o[3] = g;
    }
}

}  // namespace hmcg

namespace hmcg_host {

int ord_lds_bytes() { return (int)(sizeof(unsigned long long) * ORD_CAP); }

hipError_t launch_chain_quantiles(const OrdArgs& a, hipStream_t stream)
{
    if (a.ncols <= 0) return hipSuccess;
    if (a.Q < 1 || a.Q > HMCG_ORD_MAXQ || a.nd < 1 || a.nd > HMCG_ORD_MAXND || a.ld < a.nd || a.ncols > 0x7fffffffLL) return hipErrorInvalidValue;
    if (!a.x || !a.q || !a.n) return hipErrorInvalidValue;
    hmcg::OrdParams p{};
    p.x = a.x; p.q = a.q; p.n = reinterpret_cast<long long*>(a.n);
    p.nd = a.nd; p.ld = a.ld; p.Q = a.Q; p.round5 = a.round5 ? 1 : 0;
    for (int i = 0; i < HMCG_ORD_MAXQ; ++i) p.probs[i] = i < a.Q ? a.probs[i] : 0.0;
    hipLaunchKernelGGL(hmcg::chain_quantiles_kernel, dim3((unsigned)a.ncols), dim3(hmcg::OQ_NT), 0, stream, p);
    return hipGetLastError();
}

}  // namespace hmcg_host
