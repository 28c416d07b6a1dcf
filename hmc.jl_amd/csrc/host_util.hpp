// host_util.hpp -- the host-side pieces of libhmcgibbs.so that touch no HIP: the scatter helper threads, the chunk schedule
// of a chain, the static partition of windows over devices and the table of the per-window arrays a host-entry call
// stages (their arena layouts, the pack into pinned staging and the unpack into the caller's rows).  Plain C++17, so that the
// sanitizer builds of tests/sanitize/ (g++ -fsanitize=address,undefined / -fsanitize=thread, CPU only) compile exactly
// the code the library runs.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <numeric>
#include <thread>
#include <vector>

#include "../../include/hmcg.h"

namespace hmcg_hostutil {

// A few persistent host threads that share the scatter of a chunk (pinned staging -> the caller's arrays: 41 MB per call
// at the headline shape, as many small memcpys) with the calling thread.  On hosts whose single-thread copy rate is below
// the device's draw rate the scatter, not the GPU, would otherwise set the pace of the host entry.
class ScatterPool {
public:
    ~ScatterPool() { if (!th_.empty()) stop(); }
    void start(int workers)
    {
        if (!th_.empty() || workers <= 0) return;
        // a worker born after a stop() (hmcg_shutdown, then a new context) must not mistake the generations that went by
        // before its birth for a job: it starts from the generation current NOW (taken here, not in the thread, which may
        // first run after the first run() has already posted its job) and counts itself done only for a job it ran
        unsigned long g0;
        { std::lock_guard<std::mutex> lk(m_); g0 = gen_; }
        for (int i = 0; i < workers; ++i) th_.emplace_back([this, i, g0] { loop(i, g0); });
    }
    void stop()
    {
        { std::lock_guard<std::mutex> lk(m_); quit_ = true; ++gen_; }
        go_.notify_all();
        for (auto& t : th_) t.join();
        th_.clear();
        quit_ = false;
    }
    // f(part, nparts) for part = 0..nparts-1, nparts = workers + 1; returns when every part is done
    void run(const std::function<void(int, int)>& f)
    {
        const int np = (int)th_.size() + 1;
        if (np == 1) { f(0, 1); return; }
        { std::lock_guard<std::mutex> lk(m_); job_ = &f; pending_ = np - 1; ++gen_; }
        go_.notify_all();
        f(np - 1, np);
        std::unique_lock<std::mutex> lk(m_);
        done_.wait(lk, [this] { return pending_ == 0; });
        job_ = nullptr;
    }
private:
    void loop(int id, unsigned long seen)
    {
        for (;;) {
            const std::function<void(int, int)>* f;
            int np;
            {
                std::unique_lock<std::mutex> lk(m_);
                go_.wait(lk, [&] { return gen_ != seen; });
                seen = gen_;
                if (quit_) return;
                f = job_;
                np = (int)th_.size() + 1;
            }
            if (!f) continue;
            (*f)(id, np);
            { std::lock_guard<std::mutex> lk(m_); --pending_; }
            done_.notify_one();
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable go_, done_;
    const std::function<void(int, int)>* job_ = nullptr;
    unsigned long gen_ = 0;
    int pending_ = 0;
    bool quit_ = false;
};

// kept draws produced by the sweeps [0, g) of the sampling schedule (n_samples blocks of burnin + nrun sweeps)
inline long long kept_before(long long g, int per, int burnin, int nrun)
{
    const long long smp = g / per, i = g - smp * per;
    return smp * nrun + std::max(0LL, std::min((long long)nrun, i - burnin));
}
// global sweep index just after kept draw number d - 1 (d >= 1) has been produced
inline long long sweep_after_kept(long long d, int per, int burnin, int nrun)
{
    const long long smp = (d - 1) / nrun, i = (d - 1) - smp * nrun;
    return smp * per + burnin + i + 1;
}

struct Chunk { int s0, s1; long long d0, d1; };   // sweeps [s0, s1) produce the kept draws [d0, d1)

// Chunks of the sweep range [sb, se): draw counts halve from chunk to chunk down to ~1/32 of the run (the last chunk's
// copy-out is the only one not hidden behind sampling), never more than `cap` draws in a chunk.  fdiv_env / keep_env:
// diagnostic overrides of the 32 and of the share a chunk takes ("num/den"), nullptr in production (hmcg.hip, diag_env).
inline std::vector<Chunk> plan_chunks(int sb, int se, int per, int burnin, int nrun, long long cap, bool stream_draws,
                                      const char* fdiv_env = nullptr, const char* keep_env = nullptr)
{
    std::vector<Chunk> out;
    const long long dB = kept_before(sb, per, burnin, nrun), dE = kept_before(se, per, burnin, nrun);
    const long long nd = dE - dB;
    if (!stream_draws || nd <= 0 || se <= sb) { out.push_back({sb, se, dB, dE}); return out; }
    long long fdiv = 32;       // (measured at the headline shape: 1/8 5.34 ms, 1/16 5.30, 1/32 5.23 per call)
    if (const char* e = fdiv_env) { const long long v = atoll(e); if (v >= 2 && v <= 1024) fdiv = v; }
    const long long floor_sz = std::max(16LL, nd / fdiv);
    // share of the remaining draws a chunk takes: 2/3 (four launches at the headline shape: 667, 222, 74, 37 draws).  Until
    // the chunk copies set out on time (round 4, KernelParams::skip_host) 1/2 measured better -- its smaller first chunk hid
    // the late first copy; now every relaunch saved is ~30 us (profiles/r04/trace_host_entry_skip_words.txt)
    long long keep_num = 2, keep_den = 3;
    if (const char* e = keep_env) {
        long long a = 0, b = 0;
        if (sscanf(e, "%lld/%lld", &a, &b) == 2 && a >= 1 && b > a && b <= 64) { keep_num = a; keep_den = b; }
    }
    long long d = dB;
    int s = sb;
    while (d < dE) {
        const long long rem = dE - d;
        long long take = std::min(cap, std::max((rem * keep_num + keep_den - 1) / keep_den, floor_sz));
        if (rem - take < floor_sz / 2) take = std::min(cap, rem);       // no crumbs
        take = std::min(take, rem);
        const long long d1 = d + take;
        const int s1 = d1 == dE ? se : (int)sweep_after_kept(d1, per, burnin, nrun);
        out.push_back({s, s1, d, d1});
        d = d1; s = s1;
    }
    if (out.back().s1 != se) out.back().s1 = se;
    return out;
}

// Static LPT partition (as hmc.jl_amd/shard.py partition_windows): windows by length, longest first (stable), each to
// the lightest device that still has room under the count cap ceil(W / G).
inline std::vector<std::vector<int32_t>> partition_windows(const int32_t* T, int W, int G)
{
    std::vector<int32_t> order((size_t)W);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return T[a] > T[b]; });
    std::vector<long long> load((size_t)G, 0);
    std::vector<int> count((size_t)G, 0);
    std::vector<std::vector<int32_t>> parts((size_t)G);
    const int cap = (W + G - 1) / G;
    for (int32_t w : order) {
        int best = -1;
        for (int r = 0; r < G; ++r)
            if (count[(size_t)r] < cap && (best < 0 || load[(size_t)r] < load[(size_t)best])) best = r;
        parts[(size_t)best].push_back(w);
        load[(size_t)best] += T[w];
        ++count[(size_t)best];
    }
    for (auto& p : parts) std::sort(p.begin(), p.end());
    return parts;
}

// ---- the per-window arrays of a host-entry call ----
// offsets into an arena, 256-byte aligned; pointers are taken after the arena has grown to `total`
struct Layout {
    size_t total = 0;
    size_t add(size_t bytes) { const size_t off = total; total += (bytes + 255) & ~(size_t)255; return off; }
};

struct HostArrays {           // the caller's arrays of a host-entry call
    const double* Y; const int32_t* T; const double* yreal;
    double* mu; double* sig2; double* A; double* pi_end; double* fcast; double* summary; int32_t* status;
    const hmcg_extras* ex;
};

// The device pointers of a call, where the kernels find each array (a table row names its slot by offset); mom: the
// correlations' moment table
struct DevSlots {
    const double* Y; const int32_t* T; const double* yreal; int32_t* status; double* summary; double* mom;
    hmcg_extras ex;
};

enum BufId {
    B_Y, B_T, B_WID, B_YREAL, B_XINIT, B_SIGR, B_SAVER, B_ENDPOS, B_SIGMA,      // inputs
    B_STATUS, B_SUMMARY, B_XFINAL, B_PIF, B_SMOOTH, B_FILTER, B_SIGVALS, B_SSUM, B_MOM, B_CORR, B_XSTATE, B_SUMACC, NBUF
};
// in: sent before the first kernel.  out: returned after the last.  inout: returned, and sent on RESUME (zeroed without an array)
enum class Role : uint8_t { in, out, inout };
// Rows whose bytes are more than a copy of the caller's row.  window_id: packed as the caller's id, or window_base + g where
// the caller gives none.  resume_status: packed as the caller's status word without the skip bits (THIS call's kernel says
// what it skips), or 0.  zero_if_skipped: unpacked as zero for a skipped window (it writes nothing outside the zeroed block).
enum class Hook : uint8_t { none, window_id, resume_status, zero_if_skipped };
constexpr size_t NO_OFF = ~(size_t)0;

struct Buf {
    const char* name;
    size_t slot;        // offsetof(DevSlots, ...) of its device pointer
    Role role;
    bool zeroed;        // in the block a fresh call zeroes: an output a skipped window never writes
    bool ckpt;          // chain state (status, xstate, sumacc): on RESUME sent ahead of the other inout rows
    bool same_copy;     // returned in one copy with the row before it (adjacent on both sides)
    Hook hook;
    void* host;         // the caller's array (inputs are only read), null: none
    size_t bytes;       // per window; 0: the call does not use the array
    size_t doff = NO_OFF, poff = NO_OFF;       // offsets in the device arena and in pinned staging
    bool staged() const { return poff != NO_OFF; }
    bool sent(bool resume) const { return staged() && (role == Role::in || (resume && role == Role::inout)); }
    bool returned() const { return staged() && role != Role::in; }
};

// Both arenas open with the same INPUT block [0, input_bytes), Y at 0 (one H2D; the first half of Y sets out while the rest is
// packed).  The device arena goes on with the block a fresh call zeroes (one memset), then its other rows; pinned staging with
// the other staged rows.  Status and summary are adjacent on both sides (one small D2H).  The caller appends its own buffers.
struct BufTable {
    Buf row[NBUF];
    bool resume;
    uint32_t window_base;
    int32_t skip_mask;
    size_t input_bytes, zero_begin, zero_end;
    Layout dev, pin;
};

// The rows of a call over n windows.  need_ckpt: the chain state lives on the device (chunks, RESUME, a checkpoint asked
// for, a partial run); need_pif: the kernel streams pif through extras.pif_final whether the caller wants it or not.
inline BufTable host_buffers(const hmcg_config& cfg, const HostArrays& h, int n, bool need_ckpt, bool need_pif, size_t mom_stride)
{
    const hmcg_extras e0{};
    const hmcg_extras& x = h.ex ? *h.ex : e0;
    const size_t K = (size_t)cfg.K, ld = (size_t)cfg.ldY, H = (size_t)cfg.H, NS = 3 * K + K * K + 2 * H;
    const size_t n_samples = cfg.n_samples > 1 ? (size_t)cfg.n_samples : 1, NC = (size_t)HMCG_CORR_COLUMNS(cfg.K);
    const size_t nsv = x.sigvals && x.nsave_ld > 0 ? n_samples * (size_t)x.nsave_ld : 0;
    auto host = [](const void* p) { return const_cast<void*>(p); };
    auto when = [](bool used, size_t bytes) { return used ? bytes : 0; };
    BufTable t{};
    t.resume = (cfg.flags & HMCG_FLAG_RESUME) != 0;
    t.window_base = cfg.window_base;
    t.skip_mask = HMCG_ST_NONFINITE | HMCG_ST_BAD_T | HMCG_ST_BAD_RANGE;
    using R = Role;
    using Hk = Hook;
#define HMCG_SLOT(m) offsetof(DevSlots, m)
    //                  name              slot                          role      zeroed ckpt   same   hook                 host                       bytes (0: not used)
    t.row[B_Y]       = {"Y",              HMCG_SLOT(Y),                 R::in,    false, false, false, Hk::none,            host(h.Y),                 8 * ld};
    t.row[B_T]       = {"T",              HMCG_SLOT(T),                 R::in,    false, false, false, Hk::none,            host(h.T),                 4};
    t.row[B_WID]     = {"window_ids",     HMCG_SLOT(ex.window_ids),     R::in,    false, false, false, Hk::window_id,       host(x.window_ids),        4};
    t.row[B_YREAL]   = {"yreal",          HMCG_SLOT(yreal),             R::in,    false, false, false, Hk::none,            host(h.yreal),             when(h.yreal, 8 * H)};
    t.row[B_XINIT]   = {"x_init",         HMCG_SLOT(ex.x_init),         R::in,    false, false, false, Hk::none,            host(x.x_init),            when(x.x_init, 4 * ld)};
    t.row[B_SIGR]    = {"sig_range",      HMCG_SLOT(ex.sig_range),      R::in,    false, false, false, Hk::none,            host(x.sig_range),         when(x.sig_range, 8)};
    t.row[B_SAVER]   = {"save_range",     HMCG_SLOT(ex.save_range),     R::in,    false, false, false, Hk::none,            host(x.save_range),        when(x.save_range, 8)};
    t.row[B_ENDPOS]  = {"end_pos",        HMCG_SLOT(ex.end_pos),        R::in,    false, false, false, Hk::none,            host(x.end_pos),           when(x.end_pos, 4)};
    t.row[B_SIGMA]   = {"sigma_signal",   HMCG_SLOT(ex.sigma_signal),   R::in,    false, false, false, Hk::none,            host(x.sigma_signal),      when(x.sigma_signal, 8)};
    t.row[B_STATUS]  = {"status",         HMCG_SLOT(status),            R::inout, true,  true,  false, Hk::resume_status,   h.status,                  4};
    t.row[B_SUMMARY] = {"summary",        HMCG_SLOT(summary),           R::out,   true,  false, true,  Hk::none,            h.summary,                 when(h.summary, 8 * NS)};
    t.row[B_XFINAL]  = {"x_final",        HMCG_SLOT(ex.x_final),        R::out,   true,  false, false, Hk::none,            x.x_final,                 when(x.x_final, 4 * ld)};
    t.row[B_PIF]     = {"pif_final",      HMCG_SLOT(ex.pif_final),      R::out,   true,  false, false, Hk::none,            x.pif_final,               when(x.pif_final || need_pif, 8 * ld * K)};
    t.row[B_SMOOTH]  = {"pi_smooth_mean", HMCG_SLOT(ex.pi_smooth_mean), R::inout, true,  false, false, Hk::none,            x.pi_smooth_mean,          when(x.pi_smooth_mean, 8 * ld * K)};
    t.row[B_FILTER]  = {"pi_filter_mean", HMCG_SLOT(ex.pi_filter_mean), R::inout, true,  false, false, Hk::none,            x.pi_filter_mean,          when(x.pi_filter_mean, 8 * ld * K)};
    t.row[B_SIGVALS] = {"sigvals",        HMCG_SLOT(ex.sigvals),        R::out,   true,  false, false, Hk::none,            nsv ? x.sigvals : nullptr, 8 * nsv};
    t.row[B_SSUM]    = {"sample_summary", HMCG_SLOT(ex.sample_summary), R::inout, true,  false, false, Hk::none,            x.sample_summary,          when(x.sample_summary, 8 * n_samples * NS)};
    t.row[B_MOM]     = {"moments",        HMCG_SLOT(mom),               R::out,   false, false, false, Hk::none,            nullptr,                   when(x.corr, 8 * mom_stride)};
    t.row[B_CORR]    = {"corr",           HMCG_SLOT(ex.corr),           R::out,   false, false, false, Hk::zero_if_skipped, x.corr,                    when(x.corr, 8 * NC * NC)};
    t.row[B_XSTATE]  = {"xstate",         HMCG_SLOT(ex.xstate),         R::inout, true,  true,  false, Hk::none,            x.xstate,                  when(need_ckpt, ld)};
    t.row[B_SUMACC]  = {"sumacc",         HMCG_SLOT(ex.sumacc),         R::inout, true,  true,  false, Hk::none,            x.sumacc,                  when(need_ckpt, 8 * (NS + K))};
#undef HMCG_SLOT
    // device: the input block, the zeroed block, the rest; pinned: the input block, then the rows with a caller array (or status)
    const size_t N = (size_t)n;
    for (Buf& b : t.row) if (b.bytes && b.role == Role::in) { b.doff = t.dev.add(N * b.bytes); b.poff = t.pin.add(N * b.bytes); }
    t.input_bytes = t.zero_begin = t.dev.total;
    for (Buf& b : t.row) if (b.bytes && b.zeroed) b.doff = t.dev.add(N * b.bytes);
    t.zero_end = t.dev.total;
    for (Buf& b : t.row) {
        if (!b.bytes || b.role == Role::in) continue;
        if (!b.zeroed) b.doff = t.dev.add(N * b.bytes);
        if (b.host || b.hook == Hook::resume_status) b.poff = t.pin.add(N * b.bytes);
    }
    return t;
}

// The device pointers of the rows in use, into the arena at D.
inline DevSlots device_slots(const BufTable& t, char* D)
{
    DevSlots s{};
    s.ex.struct_size = (int32_t)sizeof(hmcg_extras);
    for (const Buf& b : t.row) {
        if (!b.bytes) continue;
        void* p = D + b.doff;
        memcpy(reinterpret_cast<char*>(&s) + b.slot, &p, sizeof p);       // every slot is a pointer member
    }
    return s;
}

// Pack windows [i0, i1) (caller rows idx[i]; idx == nullptr: row i) of every row the call sends into pinned staging at P.
inline void pack_rows(const BufTable& t, char* P, const int32_t* idx, int i0, int i1)
{
    for (int i = i0; i < i1; ++i) {
        const size_t g = idx ? (size_t)idx[i] : (size_t)i;
        for (const Buf& b : t.row) {
            if (!b.sent(t.resume)) continue;
            char* dst = P + b.poff + (size_t)i * b.bytes;
            const char* src = b.host ? static_cast<const char*>(b.host) + g * b.bytes : nullptr;
            uint32_t w = b.hook == Hook::window_id ? t.window_base + (uint32_t)g : 0;       // (4-byte rows: ids, status)
            if (src && b.hook == Hook::none) { memcpy(dst, src, b.bytes); continue; }
            if (src) memcpy(&w, src, sizeof w);
            if (b.hook == Hook::resume_status) w &= ~(uint32_t)t.skip_mask;
            memcpy(dst, &w, sizeof w);
        }
    }
}

// Unpack the returned rows of the n windows from pinned staging at P into the caller's rows.
inline void unpack_rows(const BufTable& t, const char* P, const int32_t* idx, int n)
{
    const int32_t* status = reinterpret_cast<const int32_t*>(P + t.row[B_STATUS].poff);
    for (int i = 0; i < n; ++i) {
        const size_t g = idx ? (size_t)idx[i] : (size_t)i;
        for (const Buf& b : t.row) {
            if (!b.returned() || !b.host) continue;
            char* dst = static_cast<char*>(b.host) + g * b.bytes;
            if (b.hook == Hook::zero_if_skipped && (status[i] & t.skip_mask)) memset(dst, 0, b.bytes);
            else memcpy(dst, P + b.poff + (size_t)i * b.bytes, b.bytes);
        }
    }
}

}  // namespace hmcg_hostutil
