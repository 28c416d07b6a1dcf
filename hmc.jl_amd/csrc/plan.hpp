// plan.hpp -- what a call runs: the tables of compiled kernel instantiations (types here, rows in the variants_*.hip units),
// the call's sweep schedule, and make_plan(): the argument rules of hmcg_extras, the register-resident variant, the cut of a
// ragged batch into length buckets, the LDS-resident fallback.  Integer logic over tables it is handed: plain C++17 without a
// HIP header, so that tests/sanitize/host_harness.cpp runs exactly the code the library runs, on tables of its own, on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/hmcg.h"

namespace hmcg { struct KernelParams; }       // gibbs_device.hpp; here it only appears in the kernels' signatures

namespace hmcg_host {

using KernelFn = void (*)(const hmcg::KernelParams);

struct Variant {
    int K, L, NT;
    KernelFn fn;
    bool sig, smooth;
    int NH;                // helper waves on top of the NT window threads (block = NT + 64*NH threads)
    int occ;               // 2: registers capped so that two plain blocks share a CU
    int pref_small;        // flavour to run when every window has a CU to itself (W <= CU count)
    int pref_big;          // flavour for larger batches
};
// flavours: P1 = plain, whole register file; P2 = plain, two blocks per CU; H = four helper waves
enum { P1 = 0, P2 = 1, H = 2 };
inline int flavour_of(const Variant& v) { return v.NH > 0 ? H : (v.occ == 2 ? P2 : P1); }
inline int flavour_code(const char* f) { return !strcmp(f, "h") ? H : (!strcmp(f, "p2") ? P2 : P1); }

struct VariantGroup {
    const Variant* v;
    int n;
};
// register-resident kernels (gibbs_device.hpp): base path by K, signal path, smoothed-probability path
extern const VariantGroup g_group_k2, g_group_k3, g_group_mid, g_group_k3_l16, g_group_k4, g_group_sig, g_group_smooth, g_group_sigsmooth;

using BigKernelFn = void (*)(const hmcg::KernelParams, const int);
struct BigVariant {
    int K, NT;
    BigKernelFn fn;
};
// LDS-resident kernels (gibbs_big.hpp): large K, or windows too long for the register-resident variants.  Every form --
// signal path, smoothing pass, HBM-streaming -- is compiled for K = 2..8: g_big[sig][smooth][stream][K - 2], filled by the
// variants_big*.hip units.
constexpr int BIG_KMIN = 2, BIG_NK = 7;
using BigForm = BigVariant[BIG_NK];
extern const BigForm* const g_big[2][2][2];
// the forms, one per [sig][smooth][stream]
extern const BigForm g_big_000, g_big_001, g_big_010, g_big_011, g_big_100, g_big_101, g_big_110, g_big_111;

// The tables make_plan chooses from (the library: the eight groups and g_big above).
struct KernelTables {
    const VariantGroup* const* groups;
    int ngroups;
    const BigForm* const (*big)[2][2];
};

// The sweeps of a call: n_samples chains of burnin + nrun sweeps each, of which this call runs [sweep_begin, sweep_end).
struct SweepSchedule {
    int n_samples, per_sample;                     // chains (>= 1), and the sweeps of one: burnin + nrun (>= 1: the kernels divide by it)
    int total_sweeps, nd;                          // the whole run: sweeps, and kept draws per window
    int sweep_begin, sweep_end, final_launch;      // this call's share of it; 1: it ends the run
};
inline SweepSchedule sweep_schedule(const hmcg_config& cfg)
{
    SweepSchedule s{};
    s.n_samples = std::max(1, cfg.n_samples);
    s.per_sample = std::max(1, cfg.burnin + cfg.nrun);
    s.total_sweeps = s.n_samples * (cfg.burnin + cfg.nrun);
    s.nd = s.n_samples * cfg.nrun;
    s.sweep_begin = cfg.sweep_base;
    s.sweep_end = s.total_sweeps;
    if (cfg.sweep_count > 0 && cfg.sweep_count < s.sweep_end - cfg.sweep_base) s.sweep_end = cfg.sweep_base + cfg.sweep_count;
    s.final_launch = s.sweep_end == s.total_sweeps ? 1 : 0;
    return s;
}

constexpr int MAXBUCKET = 8;       // length buckets of one call (steps-per-thread classes 1, 2, 3, 4, 6, 8, 12, 16)
constexpr int MAXCLASS = 16;       // steps-per-thread classes of one path that the cut looks at (further ones are ignored)

// What runs: the kernel instantiation for this call's shape, chosen once per call.
// One length bucket of a call: the windows with t_lo <= T <= t_hi run on variant v (its own launch, beside the others).
// Both bounds are inclusive: the first bucket reaches INT32_MAX, the last starts AT INT32_MIN, so every T lies in exactly one.
struct Bucket {
    const Variant* v;
    int t_lo, t_hi;
};
struct Plan {
    const Variant* v = nullptr;    // register-resident kernel (with buckets: the longest bucket's variant)
    int nb = 0;                    // > 1: length-bucketed dispatch, longest bucket first
    Bucket b[MAXBUCKET];
    const BigVariant* bv = nullptr;
    int bigL = 0;
    bool stream = false;           // the LDS-resident kernel's HBM-streaming form (window too long for the CU's LDS)
    size_t dyn = 0;
    bool use_sig = false, use_smooth = false;
    SweepSchedule sched{};
    bool needs_pif() const { return bv != nullptr && use_smooth; }   // the LDS-resident smoothing kernel streams pif through pif_final
    int NT() const { return v ? v->NT : bv->NT; }
    int L() const { return v ? v->L : bigL; }
    int NH() const { return v ? v->NH : 0; }
    const void* fptr() const { return v ? reinterpret_cast<const void*>(v->fn) : reinterpret_cast<const void*>(bv->fn); }
};

// Diagnostic overrides of the choice, every one unset in production (hmcg.hip fills them from the HMCG_DIAG=1 environment).
struct PlanOverrides {
    const char* flavour = nullptr;           // HMCG_FLAVOUR=p1|p2|h: that flavour whatever the table prefers (tools/variant_sweep.py)
    const char* bucket_flavours = nullptr;   // HMCG_BUCKET_FLAVOURS="h,p2,p2": per bucket, longest bucket first
    bool force_big = false;                  // HMCG_FORCE_BIG: the LDS-resident kernel also where a register-resident variant exists
    bool no_buckets = false;                 // HMCG_NO_BUCKETS: one launch sized for the longest window
    bool force_stream = false;               // HMCG_FORCE_STREAM: the LDS-resident kernel's HBM-streaming form whatever fits the LDS
    bool stamps = false;                     // the HMCG_STAMPS build: one launch (its stamp buffer describes one kernel)
};

// The window lengths of a call as the host entries know them (rows idx[0..n) of T; idx == nullptr: rows 0..n-1).
struct HostLengths {
    const int32_t* T = nullptr;
    const int32_t* idx = nullptr;
    int n = 0;
    int at(int i) const { return T[idx ? (size_t)idx[i] : (size_t)i]; }
};

// ---- step 1: the extras against the config.  nullptr, or the message that goes with HMCG_E_BADARG ----
inline const char* check_extras(const hmcg_config& cfg, const hmcg_extras* ex, const SweepSchedule& s)
{
    if (ex && ex->struct_size != (int32_t)sizeof(hmcg_extras)) return "hmcg_extras.struct_size mismatch";
    const bool resume = (cfg.flags & HMCG_FLAG_RESUME) != 0, use_sig = ex && ex->sig_range;
    if (resume && !(ex && ex->xstate)) return "HMCG_FLAG_RESUME needs extras.xstate";
    if (!use_sig && (s.n_samples > 1 || (ex && (ex->sigma_signal || ex->sigvals)))) return "n_samples / sigma_signal / sigvals need extras.sig_range";
    if (!use_sig && (cfg.blend_mask != 0 || (ex && ex->end_pos))) return "blend_mask / end_pos need extras.sig_range";
    if (cfg.blend_mask < 0 || (cfg.H < 31 && (cfg.blend_mask >> cfg.H) != 0)) return "blend_mask has bits beyond H";
    if (ex && ex->sigvals && ex->nsave_ld < 1) return "sigvals needs nsave_ld >= 1";
    if (!use_sig && ex && ex->sample_summary) return "sample_summary needs extras.sig_range (without the signal path it is `summary`)";
    if (ex && ex->corr) {
        if (use_sig || s.n_samples > 1 || cfg.H < 1 || cfg.nrun < 2)
            return "extras.corr: base runs only (no signal path), H >= 1 (the forecast column) and nrun >= 2";
        if (resume || cfg.sweep_base != 0 || (cfg.sweep_count > 0 && cfg.sweep_count < cfg.burnin + cfg.nrun))
            return "extras.corr needs the whole run in one call (no RESUME / sweep_base / sweep_count)";
    }
    if (cfg.sweep_base > s.total_sweeps) return "sweep_base beyond the run";
    return nullptr;
}

// ---- step 2: the register-resident variant ----
// The rows compiled for (K, threads per window, path), in table order: what both the variant choice and the class list read.
struct Candidates {
    const Variant* row[3 * MAXCLASS];          // (every class in three flavours; further rows are ignored, as further classes are)
    int n = 0;
    Candidates(const KernelTables& tab, int K, int nt, bool sig, bool smooth)
    {
        for (int g = 0; g < tab.ngroups; ++g)
            for (int i = 0; i < tab.groups[g]->n; ++i) {
                const Variant& v = tab.groups[g]->v[i];
                if (v.K == K && v.NT == nt && v.sig == sig && v.smooth == smooth && n < 3 * MAXCLASS) row[n++] = &v;
            }
    }
};
// The variant for a window of maxT steps: the fewest steps per thread that cover it; among those rows the flavour wanted --
// `force` (>= 0, diagnostics) or the row's preference for the batch size --, else P1, else the first; of equals the last.
inline const Variant* pick_variant(const Candidates& c, int maxT, bool small_batch, int force)
{
    const Variant* best = nullptr;
    for (int i = 0; i < c.n; ++i) {
        const Variant& v = *c.row[i];
        if (v.L * v.NT < maxT) continue;
        const int want = force >= 0 ? force : (small_batch ? v.pref_small : v.pref_big);
        auto rank = [want](const Variant& r) { return flavour_of(r) == want ? 0 : (flavour_of(r) == P1 ? 1 : 2); };
        if (!best || v.L < best->L || (v.L == best->L && rank(v) < 2 && rank(v) <= rank(*best))) best = &v;
    }
    return best;
}

// ---- step 3: the length buckets ----
// Length-bucketed dispatch: a batch of ragged windows (the reference's production run: 460 expanding windows of 120..579
// months, code/run_hmm.jl:79-109) is cut by the steps-per-thread class each window needs; every class gets its own launch
// on its own stream, all of them over the whole grid -- the blocks of the other classes' windows leave at once
// (the class bounds in the header of KernelParams::order).  A window then runs on the variant its own length selects, whatever
// else the call holds: its result equals that of a call with this window alone, bit for bit.
// c: the 256-thread rows of the path.  minT < maxT: the shortest and the longest window.  hl (host entries): the lengths
// themselves -- classes no window falls in are not launched.  Leaves pl alone where one class holds every window.
inline void cut_buckets(const Candidates& c, int minT, int maxT, const HostLengths* hl, bool small_batch, int force, const char* bucket_flavours, Plan& pl)
{
    int Ls[MAXCLASS], nL = 0;                  // the steps-per-thread classes compiled for the path, ascending
    for (int i = 0; i < c.n; ++i)
        if (std::find(Ls, Ls + nL, c.row[i]->L) == Ls + nL && nL < MAXCLASS) Ls[nL++] = c.row[i]->L;
    std::sort(Ls, Ls + nL);
    int lo = 0, hi = 0;
    while (lo < nL && 256 * Ls[lo] < minT) ++lo;
    while (hi < nL && 256 * Ls[hi] < maxT) ++hi;
    if (hi >= nL || lo >= hi) return;
    // classes that are launched, longest first: all of them on the device entry (it does not see T); on the host
    // entries only those a window falls in (the longest one always: it reports, and flags T > max_T)
    int keep[MAXCLASS], nk = 0;
    for (int k = hi; k >= lo; --k) {
        bool any = !hl || k == hi;
        const int k_lo = k == 0 ? 0 : 256 * Ls[k - 1], k_hi = 256 * Ls[k];
        for (int i = 0; hl && i < hl->n && !any; ++i) any = hl->at(i) > k_lo && hl->at(i) <= k_hi;
        if (any) keep[nk++] = k;
    }
    nk = std::min(nk, MAXBUCKET);              // (more classes than slots: the last slot's class takes every shorter window too)
    const char* bf = bucket_flavours;
    for (int j = 0; j < nk; ++j) {
        int f = force;
        if (bf && *bf) {
            char tok[8] = "";
            const size_t n = strcspn(bf, ",");
            memcpy(tok, bf, std::min(n, sizeof tok - 1));
            f = flavour_code(tok);
            bf += n + (bf[n] == ',' ? 1 : 0);
        }
        // bucket j: windows longer than the next kept class holds, up to what this class holds (a skipped class is
        // empty, so every window still runs on the smallest class that covers it)
        const int t_hi = j == 0 ? INT32_MAX : 256 * Ls[keep[j]], t_lo = j == nk - 1 ? INT32_MIN : 256 * Ls[keep[j + 1]] + 1;
        pl.b[pl.nb++] = Bucket{pick_variant(c, 256 * Ls[keep[j]], small_batch, f), t_lo, t_hi};
    }
    if (pl.nb == 1) pl.nb = 0;                 // one class after all: a plain single launch
    pl.v = pl.b[0].v;
}

// ---- step 4: the LDS-resident kernel (large K, or a window too long for the register-resident variants) ----
// static_lds(const BigVariant&): the static LDS of that instantiation (hmcg.hip asks the HIP runtime).  Leaves pl.bv null
// where no form serves the call.
template <class StaticLds>
void choose_big(const KernelTables& tab, const hmcg_config& cfg, int maxT, bool force_stream, const StaticLds& static_lds, Plan& pl)
{
    if (cfg.K < BIG_KMIN || cfg.K >= BIG_KMIN + BIG_NK) return;
    auto form = [&](bool stream) { return &(*tab.big[pl.use_sig][pl.use_smooth][stream])[cfg.K - BIG_KMIN]; };
    const BigVariant* bv = form(false);
    if (cfg.threads_per_window != 0 && cfg.threads_per_window != bv->NT) return;
    pl.bv = bv;
    pl.bigL = (maxT + bv->NT - 1) / bv->NT;
    pl.dyn = (size_t)bv->NT * pl.bigL * (8 + 8 + 4 + 1) + 16;
    // dynamic + static LDS of the instantiation must fit the CU's 160 KiB; too long for that: the same kernel with its
    // per-step arrays in an HBM scratch
    if (pl.dyn + static_lds(*bv) > 160 * 1024 || force_stream) {
        pl.bv = form(true);
        pl.stream = true;
        pl.dyn = 16;
    }
}

// Argument checks common to both entries + kernel choice.  W is the number of windows THIS device runs; minT the shortest
// of them when the caller knows it (0: unknown -- one launch sized for the longest window); hl (host entries) the lengths
// themselves.  Returns 0 and *plan, or an HMCG_E_* code and its message in err.
template <class StaticLds>
int make_plan(const KernelTables& tab, const hmcg_config& cfg, const hmcg_extras* ex, int W, int cu_count, int minT, const HostLengths* hl,
              const PlanOverrides& ov, const StaticLds& static_lds, Plan* plan, char* err, size_t nerr)
{
    Plan pl;
    pl.sched = sweep_schedule(cfg);
    if (const char* msg = check_extras(cfg, ex, pl.sched)) { snprintf(err, nerr, "%s", msg); return HMCG_E_BADARG; }
    pl.use_sig = ex && ex->sig_range != nullptr;
    pl.use_smooth = ex && (ex->pi_smooth_mean != nullptr || ex->pi_filter_mean != nullptr || ex->pi_smooth_draws != nullptr);
    const int maxT = cfg.max_T > 0 ? cfg.max_T : cfg.ldY;
    // Flavour: helper waves pay off while every window has a CU to itself; with more windows than CUs the capped
    // plain variant lets two windows share a CU instead (a helped block takes the whole register file).
    const bool small_batch = W <= cu_count;
    const int force = ov.flavour ? flavour_code(ov.flavour) : -1;
    if (cfg.K < 5 && !ov.force_big) {
        const Candidates c(tab, cfg.K, cfg.threads_per_window > 0 ? cfg.threads_per_window : 256, pl.use_sig, pl.use_smooth);
        pl.v = pick_variant(c, maxT, small_batch, force);
        if (pl.v && pl.v->NT == 256 && cfg.threads_per_window == 0 && minT > 0 && minT < maxT && !ov.no_buckets && !ov.stamps)
            cut_buckets(c, minT, maxT, hl, small_batch, force, ov.bucket_flavours, pl);
    }
    if (!pl.v) choose_big(tab, cfg, maxT, ov.force_stream, static_lds, pl);
    if (!pl.v && !pl.bv) {
        snprintf(err, nerr, "no kernel for K=%d max_T=%d threads_per_window=%d", cfg.K, maxT, cfg.threads_per_window);
        return HMCG_E_UNSUPPORTED;
    }
    *plan = pl;
    return 0;
}

}  // namespace hmcg_host
