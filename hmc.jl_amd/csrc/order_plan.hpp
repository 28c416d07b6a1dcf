// order_plan.hpp -- the argument rules of hmcg_chain_quantiles[_device], the order-preserving key of a draw, the digit schedule
// of the radix selection, the rank rule of a probability and the cut of the host entry's columns into upload groups.  Plain
// C++17 without a HIP header (in the manner of density_plan.hpp): a g++-compiled program runs exactly the code the library
// runs, on the CPU; the kernel calls ord_key, ord_unkey, ord_shift and ord_rank too.
//
// Key: u = bits(x'); key = (u >> 63) ? ~u : u | 2^63.  Unsigned order of the keys = the IEEE total order of the non-NaN
// doubles (-inf < .. < -0.0 < +0.0 < .. < +inf); the map is a bijection, so the selected key IS the selected value.
// Digits: the key is consumed from the top in ORD_DIGITS digits of ORD_BITS bits, digit d = (key >> ord_shift(d)) & ORD_MASK;
// a column is read once per digit consumed, and once more when the candidates are gathered early: at most ORD_DIGITS times.
// Groups: the W * C columns are numbered c + C * w; a group is a run of whole columns, every column in exactly one group.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/hmcg_order.h"
#include "stat_plan.hpp"

#ifdef __HIPCC__
#define HMCG_ORD_HD __host__ __device__ __forceinline__
#else
#define HMCG_ORD_HD inline
#endif

namespace hmcg_host {

constexpr int ORD_BITS = 8;                          // bits per digit: 256 counters per distinct prefix
constexpr int ORD_DIGITS = 64 / ORD_BITS;            // digit passes in the worst case = the most a column is read
constexpr unsigned ORD_MASK = (1u << ORD_BITS) - 1u;
constexpr int ORD_MAXT = 2 * HMCG_ORD_MAXQ;          // targets of a column: ranks j and min(j + 1, m - 1) of every probability
constexpr int ORD_CAP = 4096;                        // candidate keys one block sorts in LDS (the counters' 32 KB, reused)
static_assert(ORD_BITS * ORD_DIGITS == 64, "the digits cover the key exactly once");
static_assert(ORD_MAXT * (1 << ORD_BITS) * 4 == ORD_CAP * 8, "counters and candidates share one LDS buffer");

HMCG_ORD_HD int ord_shift(int d) { return 64 - ORD_BITS * (d + 1); }

HMCG_ORD_HD unsigned long long ord_key_of_bits(unsigned long long u) { return (u >> 63) ? ~u : (u | (1ull << 63)); }
HMCG_ORD_HD unsigned long long ord_bits_of_key(unsigned long long k) { return (k >> 63) ? (k & ~(1ull << 63)) : ~k; }
#ifndef __HIP_DEVICE_COMPILE__
inline unsigned long long ord_key(double x) { unsigned long long u; memcpy(&u, &x, 8); return ord_key_of_bits(u); }
inline double ord_unkey(unsigned long long k) { const unsigned long long u = ord_bits_of_key(k); double x; memcpy(&x, &u, 8); return x; }
#endif

// The rank rule: h = p * (m - 1), j = floor(h), g = h - j, each one rounded fp64 operation (m >= 1, 0 <= p <= 1: j <= m - 1).
struct OrdRank { long long j; double g; };
HMCG_ORD_HD OrdRank ord_rank(double p, long long m)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double top = (double)(m - 1);
    const double h = p * top;
    const double fl = floor(h);
    OrdRank r;
    r.j = (long long)fl;
    r.g = h - fl;
    return r;
}

// value of a probability from lo = x_(j), hi = x_(min(j + 1, m - 1)) and g.
HMCG_ORD_HD double ord_value(double lo, double hi, double g)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    if (g == 0.0 || lo == hi) return lo;
    const double diff = hi - lo;
    const double step = g * diff;
    const double v = lo + step;
    return v > hi ? hi : v;
}

// Host entry: columns per upload group.  A group buffer holds that many columns of nd doubles; the default keeps it near
// `target_bytes`; cap > 0 (HMCG_CHUNK_COLS) lowers it.  At least one column, at most all.
inline long long ord_group_cols(long long nd, long long ncols, long long cap, size_t target_bytes = (size_t)64 << 20)
{
    long long n = (long long)(target_bytes / (sizeof(double) * (size_t)nd));
    if (cap > 0 && cap < n) n = cap;
    if (n < 1) n = 1;
    return n < ncols ? n : ncols;
}
struct OrdGroup { long long c0, n; };                // columns [c0, c0 + n) of the W * C
inline std::vector<OrdGroup> ord_groups(long long ncols, long long group_cols)
{
    std::vector<OrdGroup> out;
    for (long long c0 = 0; c0 < ncols; c0 += group_cols) out.push_back({c0, c0 + group_cols <= ncols ? group_cols : ncols - c0});
    return out;
}

// Argument rules shared by both entries; 0 or HMCG_E_BADARG with the reason in msg.  No pointer is followed.
inline int check_quantiles(const hmcg_quantiles* p, const double* x, const double* q, const int64_t* n, char* msg, size_t nmsg)
{
    if (bad_struct(p, "hmcg_quantiles", msg, nmsg) || bad_W(p->W, msg, nmsg) || bad_C(p->C, msg, nmsg) || bad_nd(p->nd, msg, nmsg)) return HMCG_E_BADARG;
    // ranks and counters are 32-bit
    if (p->nd > HMCG_ORD_MAXND) { snprintf(msg, nmsg, "nd = %lld exceeds %lld (HMCG_ORD_MAXND): the counters are 32-bit", (long long)p->nd, HMCG_ORD_MAXND); return HMCG_E_BADARG; }
    if (bad_nd_ld(p->nd_ld, p->nd, msg, nmsg)) return HMCG_E_BADARG;
    if (p->Q < 1 || p->Q > HMCG_ORD_MAXQ) { snprintf(msg, nmsg, "Q = %d probabilities outside 1..%d", p->Q, HMCG_ORD_MAXQ); return HMCG_E_BADARG; }
    for (int i = 0; i < p->Q; ++i)
        if (!(p->probs[i] >= 0.0 && p->probs[i] <= 1.0)) { snprintf(msg, nmsg, "probs[%d] = %.17g outside [0, 1]", i, p->probs[i]); return HMCG_E_BADARG; }
    if (bad_WC(p->W, p->C, msg, nmsg)) return HMCG_E_BADARG;        // one block per (window, column)
    if (!x || !q || !n) { snprintf(msg, nmsg, "x, q and n are required"); return HMCG_E_BADARG; }
    return 0;
}

}  // namespace hmcg_host
