// density_plan.hpp -- the argument rules of hmcg_chain_density[_device], the cut of a window's draws into pieces and the split
// of its columns into groups that fit LDS.  Plain C++17 without a HIP header (in the manner of predictive_plan.hpp): a
// g++-compiled program runs exactly the code the library runs, on the CPU; dens_piece is also what the kernels call.
//
// Pieces: the union of the slab boundaries of stat_plan.hpp (multiples of PRED_SLAB, so an upload chunk of the host entry
// is a whole number of pieces) and the cut points splits [0, nd) into dens_pieces() <= pred_slabs(nd) + n_cuts pieces
// (d0, n, segment), n <= PRED_SLAB.  segment = the number of cuts <= d0: a piece of segment s lies inside the prefixes
// cuts[s], cuts[s + 1], ... and in no shorter one; draws beyond the last cut form segment n_cuts and feed the automatic range
// alone.  The list depends on nd and the cuts alone, so every float sum taken piece by piece does too.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/hmcg.h"
#include "stat_plan.hpp"

#ifdef __HIPCC__
#define HMCG_DENS_HD __host__ __device__ __forceinline__
#else
#define HMCG_DENS_HD inline
#endif

namespace hmcg_host {

constexpr int DENS_SLOTS = 3;                // counters behind the B bins: below, above, nan
constexpr int DENS_LDS_WORDS = 8192;         // 32-bit counters one block keeps in LDS (32 KB of the 160 KB a CU has)

struct DensPiece { long long d0, n; int segment; };

// A cut that opens a piece of its own: not a slab boundary already, and not the end of the draws.
HMCG_DENS_HD bool dens_proper(long long cut, long long nd) { return cut < nd && cut % PRED_SLAB != 0; }

HMCG_DENS_HD long long dens_pieces(long long nd, const int64_t* cuts, int n_cuts)
{
    long long n = (nd + PRED_SLAB - 1) / PRED_SLAB;
    for (int j = 0; j < n_cuts; ++j) n += dens_proper(cuts[j], nd) ? 1 : 0;
    return n;
}

// Index of the piece that holds draw d (0 <= d < nd); for d == nd the number of pieces.
HMCG_DENS_HD long long dens_piece_of(long long d, long long nd, const int64_t* cuts, int n_cuts)
{
    long long q = d < nd ? d / PRED_SLAB : (nd + PRED_SLAB - 1) / PRED_SLAB - 1;
    for (int j = 0; j < n_cuts; ++j) q += dens_proper(cuts[j], nd) && cuts[j] <= d ? 1 : 0;
    return d < nd ? q : q + 1;
}

// Piece q of the list, 0 <= q < dens_pieces().  In the merged list of slab starts and proper cuts, proper cut t (ascending)
// stands at index t + cuts / PRED_SLAB + 1.
HMCG_DENS_HD DensPiece dens_piece(long long q, long long nd, const int64_t* cuts, int n_cuts)
{
    long long before = 0, start = -1;
    for (int j = 0; j < n_cuts; ++j) {
        if (!dens_proper(cuts[j], nd)) continue;
        const long long idx = before + cuts[j] / PRED_SLAB + 1;
        if (idx > q) break;
        ++before;
        if (idx == q) start = cuts[j];
    }
    DensPiece p;
    p.d0 = start >= 0 ? start : (q - before) * PRED_SLAB;
    long long end = (p.d0 / PRED_SLAB + 1) * PRED_SLAB;
    if (end > nd) end = nd;
    p.segment = 0;
    for (int j = 0; j < n_cuts; ++j) {
        if (cuts[j] <= p.d0) ++p.segment;
        else if (cuts[j] < end) end = cuts[j];
    }
    p.n = end - p.d0;
    return p;
}

// Columns whose [B + 3] counters one block keeps in LDS, and the number of such groups of a call's C columns.
HMCG_DENS_HD int dens_group_cols(int C, int B)
{
    const int fit = DENS_LDS_WORDS / (B + DENS_SLOTS);
    return C < fit ? C : fit;
}
HMCG_DENS_HD int dens_groups(int C, int B)
{
    const int g = dens_group_cols(C, B);
    return (C + g - 1) / g;
}

// Argument rules shared by both entries; 0 or HMCG_E_BADARG with the reason in msg.  No device pointer is followed; host: lo_hi
// is host memory and must be finite with hi >= lo.
inline int check_density(const hmcg_density* p, const double* x, const double* lo_hi, const double* range, const int64_t* counts,
                         const double* stats, const double* trace, bool host, char* msg, size_t nmsg)
{
    if (bad_struct(p, "hmcg_density", msg, nmsg) || bad_W(p->W, msg, nmsg) || bad_C(p->C, msg, nmsg)) return HMCG_E_BADARG;
    if (p->B < 1 || p->B > HMCG_DENS_MAXBINS) { snprintf(msg, nmsg, "B = %d bins outside 1..%d", p->B, HMCG_DENS_MAXBINS); return HMCG_E_BADARG; }
    // counts are 64-bit, but n is a divisor in fp64
    if (bad_nd(p->nd, msg, nmsg) || bad_exact_nd(p->nd, msg, nmsg) || bad_nd_ld(p->nd_ld, p->nd, msg, nmsg)) return HMCG_E_BADARG;
    if (p->n_cuts < 1 || p->n_cuts > HMCG_MAXH) { snprintf(msg, nmsg, "n_cuts = %d outside 1..%d", p->n_cuts, HMCG_MAXH); return HMCG_E_BADARG; }
    for (int j = 0; j < p->n_cuts; ++j) {
        if (p->cuts[j] < 1 || p->cuts[j] > p->nd) {
            snprintf(msg, nmsg, "cut %lld outside 1..nd = %lld", (long long)p->cuts[j], (long long)p->nd);
            return HMCG_E_BADARG;
        }
        if (j > 0 && p->cuts[j] <= p->cuts[j - 1]) {
            snprintf(msg, nmsg, "cuts not strictly ascending: %lld after %lld", (long long)p->cuts[j], (long long)p->cuts[j - 1]);
            return HMCG_E_BADARG;
        }
    }
    if (p->trace_len < 0 || p->trace_len > HMCG_DENS_MAXTRACE) {
        snprintf(msg, nmsg, "trace_len = %d outside 0..%d", p->trace_len, HMCG_DENS_MAXTRACE);
        return HMCG_E_BADARG;
    }
    if (p->trace_stride < 1) { snprintf(msg, nmsg, "trace_stride = %lld: at least 1", (long long)p->trace_stride); return HMCG_E_BADARG; }
    if (p->trace_len > 0 && p->trace_stride > p->nd / p->trace_len) {
        snprintf(msg, nmsg, "trace_len * trace_stride = %d * %lld > nd = %lld", p->trace_len, (long long)p->trace_stride, (long long)p->nd);
        return HMCG_E_BADARG;
    }
    if ((long double)p->W * (long double)dens_pieces(p->nd, p->cuts, p->n_cuts) * (long double)dens_groups(p->C, p->B) > 2147483647.0L) {
        snprintf(msg, nmsg, "W * pieces * column groups exceeds one launch (2^31 - 1 blocks)");
        return HMCG_E_BADARG;
    }
    if (bad_WC(p->W, p->C, msg, nmsg)) return HMCG_E_BADARG;        // the finalize kernel
    if (!x || !range || !counts || !stats) { snprintf(msg, nmsg, "x, range, counts and stats are required"); return HMCG_E_BADARG; }
    if (!trace && p->trace_len > 0) { snprintf(msg, nmsg, "trace is NULL with trace_len > 0"); return HMCG_E_BADARG; }
    if (host && lo_hi)
        for (long long i = 0; i < (long long)p->W * p->C; ++i) {
            const double lo = lo_hi[2 * i], hi = lo_hi[2 * i + 1];
            if (!std::isfinite(lo) || !std::isfinite(hi) || !(hi >= lo)) {
                snprintf(msg, nmsg, "lo_hi[%lld] = (%g, %g): finite with hi >= lo", i, lo, hi);
                return HMCG_E_BADARG;
            }
        }
    return 0;
}

}  // namespace hmcg_host
