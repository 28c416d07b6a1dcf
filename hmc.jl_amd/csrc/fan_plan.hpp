// fan_plan.hpp -- the argument rules of hmcg_predictive_quantiles[_device], the size of its work area and the arithmetic of
// the inversion outside the CDF itself: the range term, the points of a bracket, the cell choice and the finish.  Plain C++17
// without a HIP header (in the manner of ergodic_plan.hpp): a g++-compiled program runs exactly the code the library runs, on
// the CPU; the kernels of fan.hip expand the same functions, so the two compile the same statements.
//
// Why a fixed grid refinement and not Newton: every round is the same batch of fp64 Phi evaluations for every (window, horizon,
// probability), so the launch count depends on `rounds` alone and nothing is read back; each round divides the bracket by 32
// (the first by 128) whatever the data look like, where a bracketed Newton step needs between 4 and more than 30 rounds
// depending on how far apart the regime means lie.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/hmcg_fan.h"
#include "stat_plan.hpp"

#ifdef __HIPCC__
#define HMCG_FAN_HD __host__ __device__ __forceinline__
#else
#define HMCG_FAN_HD inline
#endif

namespace hmcg_host {

constexpr int FAN_M1 = 128;              // cells of round 1: 129 points per (window, horizon)
constexpr int FAN_M = 32;                // cells of a later round: 31 interior points per (window, horizon, probability)
constexpr double FAN_Z = 40.0;           // the range reaches 40 standard deviations past every mean: Phi is exactly 0 / 1 there

inline int fan_rounds(const hmcg_fan& p) { return p.rounds == 0 ? HMCG_FAN_ROUNDS_DEFAULT : p.rounds; }
// Items (points to evaluate) per (window, horizon) and per window in round 1 and in a later round.
constexpr int fan_items_h(int n_p, bool first) { return first ? FAN_M1 + 1 : n_p * (FAN_M - 1); }
constexpr int fan_items(int n_h, int n_p, bool first) { return n_h * fan_items_h(n_p, first); }
constexpr int fan_max_items(int n_h, int n_p) { return fan_items(n_h, n_p, true) > fan_items(n_h, n_p, false) ? fan_items(n_h, n_p, true) : fan_items(n_h, n_p, false); }
// Work area: [W][nslab_total][max items] slab sums; the range pass keeps its per-slab (min, max) in the first two of a row.
inline size_t fan_part_doubles(int W, long long nd, int n_h, int n_p) { return (size_t)W * (size_t)pred_slabs(nd) * (size_t)fan_max_items(n_h, n_p); }

// Argument rules shared by both entries; 0 or HMCG_E_BADARG with the reason in msg.  No pointer but p is followed.
inline int check_fan(const hmcg_fan* p, const double* mu, const double* sig2, const double* pi_end, const double* A, const double* out,
                     const double* range, const int32_t* flag, char* msg, size_t nmsg)
{
    if (bad_struct(p, "hmcg_fan", msg, nmsg) || bad_K(p->K, msg, nmsg) || bad_W(p->W, msg, nmsg) || bad_horizons(p->n_h, p->horizons, msg, nmsg))
        return HMCG_E_BADARG;
    if (told(p->n_p < 1 || p->n_p > HMCG_FAN_MAXP, msg, nmsg, "n_p = %d probabilities outside 1..%d", p->n_p, HMCG_FAN_MAXP)) return HMCG_E_BADARG;
    for (int i = 0; i < p->n_p; ++i)
        if (told(!(std::isfinite(p->probs[i]) && p->probs[i] > 0.0 && p->probs[i] < 1.0), msg, nmsg, "probs[%d] = %g is not strictly inside (0, 1)", i,
                 p->probs[i]))
            return HMCG_E_BADARG;
    if (told(p->rounds < 0 || p->rounds > HMCG_FAN_MAXROUNDS, msg, nmsg, "rounds = %d outside 0..%d", p->rounds, HMCG_FAN_MAXROUNDS)) return HMCG_E_BADARG;
    if (bad_nd(p->nd, msg, nmsg) || bad_nd_ld(p->nd_ld, p->nd, msg, nmsg)) return HMCG_E_BADARG;
    if (told(!mu || !sig2 || !pi_end || !out || !range || !flag, msg, nmsg, "mu, sig2, pi_end, out, range and flag are required")) return HMCG_E_BADARG;
    if (told(!A && mixture_max_horizon(*p) > 0, msg, nmsg, "A is NULL with a horizon > 0")) return HMCG_E_BADARG;
    return 0;
}

// The two range terms of one (draw, state): mu -+ 40 sqrt(sig2), each step one rounded operation.
HMCG_FAN_HD void fan_reach(double mu, double sig2, double* lo, double* hi)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double sd = sqrt(sig2);
    const double r = FAN_Z * sd;
    *lo = mu - r;
    *hi = mu + r;
}

// Point m of the bracket (lo, hi) cut into M cells.
HMCG_FAN_HD double fan_point(double lo, double hi, int M, int m)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double step = (hi - lo) / (double)M;
    const double t = (double)m * step;
    return m == M ? hi : lo + t;
}

// F at point m of a bracket: round 1 holds all M + 1 values in Fs; a later round the M - 1 interior ones, the ends carried.
HMCG_FAN_HD double fan_F(const double* Fs, bool first, int M, int m, double Flo, double Fhi)
{
    return first ? Fs[m] : m == 0 ? Flo : m == M ? Fhi : Fs[m - 1];
}

// One round's cell choice for one probability: b = (lo, hi, Flo, Fhi) is replaced by the cell (y_{m*-1}, y_{m*}, F_{m*-1}, F_{m*}),
// m* the smallest m in 1..M with F(y_m) >= p, M if there is none (a NaN compares false).  In round 1 (first) the end values of
// b are not read.  Returns m*.
HMCG_FAN_HD int fan_choose(double* b, const double* Fs, bool first, double p)
{
    const int M = first ? FAN_M1 : FAN_M;
    int ms = M;
    for (int m = M - 1; m >= 1; --m) ms = fan_F(Fs, first, M, m, b[2], b[3]) >= p ? m : ms;
    const double lo = fan_point(b[0], b[1], M, ms - 1), hi = fan_point(b[0], b[1], M, ms);
    const double Flo = fan_F(Fs, first, M, ms - 1, b[2], b[3]), Fhi = fan_F(Fs, first, M, ms, b[2], b[3]);
    b[0] = lo; b[1] = hi; b[2] = Flo; b[3] = Fhi;
    return ms;
}

// The quantile read off the last bracket by inverse linear interpolation; returns the flag.
HMCG_FAN_HD int fan_finish(const double* b, double p, double* q)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double lo = b[0], hi = b[1], Flo = b[2], Fhi = b[3];
    if (Flo != Flo || Fhi != Fhi) { *q = Flo + Fhi; return HMCG_FAN_NAN; }
    const double dF = Fhi - Flo;
    if (!(dF > 0.0)) { *q = lo; return HMCG_FAN_FLAT; }
    if (p > Fhi) { *q = hi; return HMCG_FAN_UNREACHED; }
    const double r = (p - Flo) / dF;
    const double t = (hi - lo) * r;
    *q = lo + t;
    return 0;
}

}  // namespace hmcg_host
