// stat_plan.hpp -- what the draw statistics share on the host: the cut of a window's draws into slabs and upload chunks, the
// argument rules every check_* begins with, the horizon list and draw columns of the predictive mixture's four features, and
// the range rules of a launch.  Plain C++17 without a HIP header (in the manner of plan.hpp): a
// g++-compiled program runs exactly the code the library runs, on the CPU.
//
// Slabs: draws [s * PRED_SLAB, min((s + 1) * PRED_SLAB, nd)) of every window are reduced by one block in draw order; the
// slab sums are added in slab order afterwards.  The cut depends on nd alone, so the result does not depend on how the host
// entry uploads the draws: its chunks are whole slabs (the last one ends at nd).
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/hmcg.h"

namespace hmcg_host {

constexpr long long PRED_SLAB = 1024;       // draws per slab (and per block of the accumulation kernel)

inline long long pred_slabs(long long nd) { return (nd + PRED_SLAB - 1) / PRED_SLAB; }

// Host entry: draws per upload chunk.  A chunk buffer holds W * ncol columns of that many doubles; the default keeps it near
// `target_bytes`; cap > 0 (HMCG_CHUNK_DRAWS) lowers it.  Always a whole number of slabs, at least one.
inline long long pred_chunk_draws(long long nd, int W, int ncol, long long cap, size_t target_bytes = (size_t)64 << 20)
{
    long long n = (long long)(target_bytes / (sizeof(double) * (size_t)W * (size_t)ncol));
    if (cap > 0 && cap < n) n = cap;
    n = (n + PRED_SLAB - 1) / PRED_SLAB * PRED_SLAB;          // rounded UP to whole slabs
    if (n < PRED_SLAB) n = PRED_SLAB;
    const long long all = pred_slabs(nd) * PRED_SLAB;
    return n < all ? n : all;
}

struct PredChunk { long long d0, n; };       // draws [d0, d0 + n) of every window; d0 is a slab boundary
inline std::vector<PredChunk> pred_chunks(long long nd, long long chunk_draws)
{
    std::vector<PredChunk> out;
    for (long long d0 = 0; d0 < nd; d0 += chunk_draws) out.push_back({d0, d0 + chunk_draws <= nd ? chunk_draws : nd - d0});
    return out;
}

// The argument rules the check_* of the five features share, one function per rule: true when the rule is broken, with the
// reason in msg (`told`).  A check_* strings them with || in its own order and puts its own rules in between, so the first rule a
// doubly wrong call is told about is that feature's.  S: the feature's struct of include/hmcg.h, `name` its name there.
__attribute__((format(printf, 4, 5))) inline bool told(bool bad, char* msg, size_t nmsg, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    if (bad) vsnprintf(msg, nmsg, fmt, ap);
    va_end(ap);
    return bad;
}
template <class S>
inline bool bad_struct(const S* p, const char* name, char* msg, size_t nmsg)
{
    if (!p) return told(true, msg, nmsg, "%s is NULL", name);
    return told(p->struct_size != (int32_t)sizeof(S), msg, nmsg, "%s.struct_size %d != %d", name, p->struct_size, (int)sizeof(S));
}
inline bool bad_W(int W, char* msg, size_t nmsg) { return told(W < 1, msg, nmsg, "W = %d: at least one window", W); }
inline bool bad_K(int K, char* msg, size_t nmsg) { return told(K < 2 || K > HMCG_MAXK, msg, nmsg, "K = %d outside 2..%d", K, HMCG_MAXK); }
inline bool bad_nd(long long nd, char* msg, size_t nmsg) { return told(nd < 1, msg, nmsg, "nd = %lld: at least one draw", nd); }
inline bool bad_nd_ld(long long nd_ld, long long nd, char* msg, size_t nmsg) { return told(nd_ld < nd, msg, nmsg, "nd_ld = %lld < nd = %lld", nd_ld, nd); }
// ... and those that two or three of them share: the horizon list (CDFs, mixture moments; one horizon: bias moments), the
// column count, an nd that is an exact fp64 divisor and a (window, column) grid within one launch (densities, autocorrelation).
inline bool bad_horizon(int h, char* msg, size_t nmsg) { return told(h < 0 || h > HMCG_PRED_MAXH, msg, nmsg, "horizon %d outside 0..%d", h, HMCG_PRED_MAXH); }
inline bool bad_horizons(int n_h, const int32_t* horizons, char* msg, size_t nmsg)
{
    if (told(n_h < 1 || n_h > HMCG_MAXH, msg, nmsg, "n_h = %d horizons outside 1..%d", n_h, HMCG_MAXH)) return true;
    for (int j = 0; j < n_h; ++j)
        if (bad_horizon(horizons[j], msg, nmsg)) return true;
    return false;
}
inline bool bad_C(int C, char* msg, size_t nmsg) { return told(C < 1 || C > HMCG_MAXK * HMCG_MAXK, msg, nmsg, "C = %d columns outside 1..%d", C, HMCG_MAXK * HMCG_MAXK); }
inline bool bad_exact_nd(long long nd, char* msg, size_t nmsg) { return told(nd > (1LL << 53), msg, nmsg, "nd = %lld exceeds 2^53, the largest exact divisor", nd); }
inline bool bad_WC(int W, int C, char* msg, size_t nmsg) { return told((long long)W * C > 2147483647LL, msg, nmsg, "W * C exceeds one launch (2^31 - 1 blocks)"); }
// The largest of a checked horizon list (0: the transition draws are not read).
inline int max_horizon(int n_h, const int32_t* horizons)
{
    int m = 0;
    for (int j = 0; j < n_h; ++j) m = horizons[j] > m ? horizons[j] : m;
    return m;
}
// The horizon list as the kernels and launchers carry it: hz[HMCG_MAXH], zero from n_h on.  True when a horizon is > 0, that
// is when the transition draws are read.
inline bool fill_horizons(int n_h, const int32_t* horizons, int* hz)
{
    for (int j = 0; j < HMCG_MAXH; ++j) hz[j] = j < n_h ? horizons[j] : 0;
    return max_horizon(HMCG_MAXH, hz) > 0;
}
// The four features of the predictive mixture.  S: hmcg_predictive, hmcg_mixmom, hmcg_fan or hmcg_score, which name n_h and
// horizons alike: the largest horizon of a checked call ...
template <class S>
inline int mixture_max_horizon(const S& p) { return max_horizon(p.n_h, p.horizons); }
// ... and the draw columns per window a call reads: mu, sig2, pi_end (K each) and A (K * K) with a horizon > 0.
inline int mixture_columns(int K, bool with_A) { return 3 * K + (with_A ? K * K : 0); }

// A launch over slabs [slab0, slab0 + pred_slabs(nd)) of a run of nslab_total: inside the run, the arrays long enough, one
// block per (window, slab) within a grid.
inline bool slab_range_ok(int W, long long nd, long long nd_ld, long long slab0, long long nslab_total)
{
    const long long nslab = pred_slabs(nd);
    return nd_ld >= nd && slab0 >= 0 && slab0 + nslab <= nslab_total && (long long)W * nslab <= 0x7fffffffLL;
}
// A launch over draws [d_origin, d_origin + n) of a run of nd: it starts on a slab boundary, ends inside the run, and a chunk
// that is not the last is whole slabs.
inline bool chunk_origin_ok(long long d_origin, long long n, long long nd)
{
    if (n < 1 || d_origin < 0 || d_origin % PRED_SLAB != 0 || d_origin + n > nd) return false;
    return d_origin + n == nd || n % PRED_SLAB == 0;
}

}  // namespace hmcg_host
