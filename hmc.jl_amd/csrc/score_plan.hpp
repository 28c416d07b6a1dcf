// score_plan.hpp -- everything of hmcg_predictive_scores[_device] that is not a kernel: the thinning, the cut of the component
// square into tiles and blocks, the row pairing, the work area, the window groups of the host entry, the argument rules, and
// the per-term arithmetic a(m, S2) the kernels of score.hip expand.  Plain C++17 without a HIP header (in the manner of
// fan_plan.hpp): a g++-compiled program runs exactly the code the library runs, on the CPU.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/hmcg_score.h"
#include "stat_plan.hpp"

#ifdef __HIPCC__
#define HMCG_SCORE_HD __host__ __device__ __forceinline__
#else
#define HMCG_SCORE_HD inline
#endif

namespace hmcg_host {

constexpr int SCORE_TP = 256;            // components per tile of the pair pass = threads of its block = one block's row share

// Thinning: the stride a call uses and the draws it leaves.
inline long long score_stride(long long nd, long long stride)
{
    return stride > 0 ? stride : (nd + HMCG_SCORE_DRAWS_DEFAULT - 1) / HMCG_SCORE_DRAWS_DEFAULT;
}
inline long long score_used(long long nd, long long stride) { const long long s = score_stride(nd, stride); return (nd + s - 1) / s; }
inline long long score_used(const hmcg_score& p) { return score_used(p.nd, p.stride); }

// The component square: N = n_u * K components in nT tiles; block b takes the tile rows b and nT - 1 - b (rows r hold r + 1
// tiles, so every block carries nT + 1 of them; the middle row of an odd nT stands alone).
inline long long score_comps(long long n_u, int K) { return n_u * (long long)K; }
inline long long score_tiles(long long N) { return (N + SCORE_TP - 1) / SCORE_TP; }
inline long long score_blocks(long long N) { return (score_tiles(N) + 1) / 2; }
HMCG_SCORE_HD int score_rows(long long nT, long long b, long long* r) { r[0] = b; r[1] = nT - 1 - b; return r[0] == r[1] ? 1 : 2; }

// Work area of one window, in doubles: mu[N] | sig2[N] | omega[n_h][N] | linear slab sums [slabs][3 n_h] (F, E, P by horizon) |
// pair partials [blocks][n_h].
struct ScoreWork { size_t o_mu, o_v, o_w, o_lin, o_pair, total; };
inline ScoreWork score_work(long long n_u, int K, int n_h)
{
    const size_t N = (size_t)score_comps(n_u, K);
    ScoreWork s{};
    s.o_mu = 0; s.o_v = N; s.o_w = 2 * N; s.o_lin = s.o_w + (size_t)n_h * N;
    s.o_pair = s.o_lin + (size_t)pred_slabs(n_u) * 3 * (size_t)n_h;
    s.total = s.o_pair + (size_t)score_blocks((long long)N) * (size_t)n_h;
    return s;
}
inline size_t score_work_doubles(int W, long long n_u, int K, int n_h) { return (size_t)W * score_work(n_u, K, n_h).total; }

// Host entry: windows per upload group.  A staging buffer holds that many windows of ncol columns of n_u doubles; the default
// keeps it near `target_bytes`; cap > 0 (HMCG_SCORE_GROUP_WINDOWS) lowers it.  At least one window.
inline int score_group_windows(int W, long long n_u, int ncol, long long cap, size_t target_bytes = (size_t)64 << 20)
{
    long long g = (long long)(target_bytes / (sizeof(double) * (size_t)ncol * (size_t)n_u));
    if (cap > 0 && cap < g) g = cap;
    if (g < 1) g = 1;
    return g < W ? (int)g : W;
}

// Argument rules shared by both entries; 0 or HMCG_E_BADARG with the reason in msg.  No pointer but p is followed.
inline int check_score(const hmcg_score* p, const double* mu, const double* sig2, const double* pi_end, const double* A, const double* yreal,
                       const double* out, char* msg, size_t nmsg)
{
    if (bad_struct(p, "hmcg_score", msg, nmsg) || bad_K(p->K, msg, nmsg) || bad_W(p->W, msg, nmsg) || bad_horizons(p->n_h, p->horizons, msg, nmsg))
        return HMCG_E_BADARG;
    if (bad_nd(p->nd, msg, nmsg) || bad_nd_ld(p->nd_ld, p->nd, msg, nmsg)) return HMCG_E_BADARG;
    if (told(p->stride < 0, msg, nmsg, "stride = %lld is negative", (long long)p->stride)) return HMCG_E_BADARG;
    const long long n_u = score_used(*p), nblk = score_blocks(score_comps(n_u, p->K)), nslab = pred_slabs(n_u);
    if (told((long long)p->W * (nblk > nslab ? nblk : nslab) > 2147483647LL, msg, nmsg, "W * blocks per window exceeds one launch (2^31 - 1 blocks)"))
        return HMCG_E_BADARG;
    if (told(!mu || !sig2 || !pi_end || !yreal || !out, msg, nmsg, "mu, sig2, pi_end, yreal and out are required")) return HMCG_E_BADARG;
    if (told(!A && mixture_max_horizon(*p) > 0, msg, nmsg, "A is NULL with a horizon > 0")) return HMCG_E_BADARG;
    return 0;
}

constexpr double SCORE_SQRT2 = 1.4142135623730951;
constexpr double SCORE_SQRT_2_PI = 0.7978845608028654;       // sqrt(2 / pi)
constexpr double SCORE_INV_SQRT_PI = 0.5641895835477563;     // 1 / sqrt(pi)

// E|Z| of Z ~ N(m, S2), each step one rounded operation (include/hmcg_score.h states the order).
HMCG_SCORE_HD double score_a(double m, double S2)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    if (S2 == 0.0) return fabs(m);
    const double s = sqrt(S2);
    const double d = SCORE_SQRT2 * s;
    const double r = 1.0 / d;
    const double t = m * r;
    const double e = erf(t);
    const double t2 = t * t;
    const double g = exp(-t2);
    const double p1 = m * e;
    const double q = s * SCORE_SQRT_2_PI;
    const double p2 = q * g;
    return p1 + p2;
}

// The three per-component values of the linear pass at the point y: Phi, a and the density (c = 1 / (sqrt(2) sqrt(sig2)), as
// the CDF entry stages it).
HMCG_SCORE_HD void score_point(double y, double mu, double sig2, double c, double* ph, double* ak, double* dk)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double m = y - mu;
    const double t = m * c;
    *ph = 0.5 * erfc(-t);
    *ak = score_a(m, sig2);
    const double t2 = t * t;
    const double g = exp(-t2);
    const double q = c * SCORE_INV_SQRT_PI;
    *dk = q * g;
}

}  // namespace hmcg_host
