// Sanitizer harness for the host-side code of libhmcgibbs.so that needs no GPU (tests/test_sanitizers.py builds it with
// g++ -fsanitize=address,undefined and with -fsanitize=thread and runs it on the CPU):
//   * hmcg_hostutil::ScatterPool -- the helper threads of the host entry's scatter: start / run / stop / start again with a
//     job posted at once (the generation race of ADVICE r2), many jobs, jobs that write disjoint parts of one array;
//   * hmcg_hostutil::partition_windows, plan_chunks -- invariants on random shapes;
//   * hmcg_hostutil::host_buffers, pack_rows, unpack_rows -- the table of a host-entry call's per-window arrays on random
//     configurations: the arena layouts' invariants, and pack + unpack against the caller's rows;
//   * hmcg_host::make_plan, sweep_schedule (csrc/plan.hpp) -- which kernel a call runs and how a ragged batch is cut into length
//     buckets, on tables built here, against a brute-force restatement: every int32_t length in exactly one bucket, the class
//     and flavour of every launch, the LDS-resident fallback and its LDS fit, every argument rule's message, the sweep range;
//   * hmcg_csv.cpp -- hmcg_format_float, hmcg_write_table_csv and hmcg_save_results_csv with its thread pool.
// Exits 0 when every check holds; sanitizer reports make it exit non-zero by themselves.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <sys/stat.h>

#include "../../hmc.jl_amd/csrc/host_util.hpp"
#include "../../hmc.jl_amd/csrc/plan.hpp"
#include "../../include/hmcg.h"

using namespace hmcg_hostutil;
using namespace hmcg_host;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); return 1; } } while (0)

static int pool_checks()
{
    std::vector<double> src(1 << 18), dst(1 << 18);
    for (size_t i = 0; i < src.size(); ++i) src[i] = (double)i * 0.5;
    for (int round = 0; round < 40; ++round) {
        ScatterPool pool;
        pool.start(round % 4);                              // 0..3 helpers
        const int jobs = round < 8 ? 1 : 25;                // the first rounds post their only job right after start()
        for (int j = 0; j < jobs; ++j) {
            std::fill(dst.begin(), dst.end(), -1.0);
            const std::function<void(int, int)> part = [&](int pi, int np) {
                const size_t n = src.size(), i0 = n * (size_t)pi / (size_t)np, i1 = n * (size_t)(pi + 1) / (size_t)np;
                memcpy(dst.data() + i0, src.data() + i0, 8 * (i1 - i0));
            };
            pool.run(part);
            CHECK(memcmp(dst.data(), src.data(), 8 * src.size()) == 0);       // every part done when run() returns
        }
        pool.stop();
        pool.start(3);                                      // same object again: generation counter has moved on
        int hits[4] = {0, 0, 0, 0};
        const std::function<void(int, int)> count = [&](int pi, int np) { (void)np; hits[pi] += 1; };
        pool.run(count);
        CHECK(hits[0] == 1 && hits[1] == 1 && hits[2] == 1 && hits[3] == 1);
        pool.stop();
    }
    return 0;
}

static int partition_checks()
{
    std::mt19937 g(7);
    for (int rep = 0; rep < 300; ++rep) {
        const int W = 1 + (int)(g() % 700), G = 1 + (int)(g() % 8);
        std::vector<int32_t> T((size_t)W);
        for (auto& t : T) t = 2 + (int32_t)(g() % 5000);
        const int Gu = std::min(G, W);
        const auto parts = partition_windows(T.data(), W, Gu);
        CHECK((int)parts.size() == Gu);
        std::vector<int> seen((size_t)W, 0);
        const int cap = (W + Gu - 1) / Gu;
        long long lo = 1LL << 60, hi = 0;
        for (const auto& p : parts) {
            CHECK((int)p.size() <= cap);
            long long load = 0;
            for (size_t i = 0; i < p.size(); ++i) { CHECK(p[i] >= 0 && p[i] < W); seen[(size_t)p[i]]++; load += T[(size_t)p[i]]; CHECK(i == 0 || p[i - 1] < p[i]); }
            lo = std::min(lo, load); hi = std::max(hi, load);
        }
        for (int s : seen) CHECK(s == 1);
        if (W >= 4 * Gu) CHECK(hi - lo <= 2 * 5002LL + (hi / 4));       // LPT under a count cap: loads stay close
    }
    return 0;
}

static int chunk_checks()
{
    std::mt19937 g(11);
    for (int rep = 0; rep < 2000; ++rep) {
        const int burnin = (int)(g() % 50), nrun = (int)(g() % 400), ns = 1 + (int)(g() % 4);
        const int per = std::max(1, burnin + nrun), total = ns * (burnin + nrun);
        int sb = total > 0 ? (int)(g() % (unsigned)(total + 1)) : 0, se = total;
        if (g() & 1) se = sb + (int)(g() % (unsigned)(total - sb + 1));
        const long long cap = 1 + (long long)(g() % 300);
        const bool stream = (g() % 4) != 0;
        const auto ch = plan_chunks(sb, se, per, burnin, nrun, cap, stream);
        CHECK(!ch.empty() && ch.front().s0 == sb && ch.back().s1 == se);
        CHECK(ch.front().d0 == kept_before(sb, per, burnin, nrun) && ch.back().d1 == kept_before(se, per, burnin, nrun));
        for (size_t i = 0; i < ch.size(); ++i) {
            CHECK(ch[i].s0 <= ch[i].s1 && ch[i].d0 <= ch[i].d1);
            if (i) CHECK(ch[i].s0 == ch[i - 1].s1 && ch[i].d0 == ch[i - 1].d1);
            CHECK(kept_before(ch[i].s1, per, burnin, nrun) - kept_before(ch[i].s0, per, burnin, nrun) == ch[i].d1 - ch[i].d0);
            if (stream && ch.size() > 1) CHECK(ch[i].d1 - ch[i].d0 <= cap);
        }
    }
    return 0;
}

static size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

// The layouts of host_buffers on random configurations, and pack_rows + unpack_rows against the caller's rows.
static int buffer_checks()
{
    std::mt19937 g(13);
    auto coin = [&]() { return (g() & 1) != 0; };
    const BufId zeroed_ids[] = {B_STATUS, B_SUMMARY, B_XSTATE, B_SUMACC, B_XFINAL, B_SIGVALS, B_SSUM, B_PIF, B_SMOOTH, B_FILTER};
    const BufId resume_ids[] = {B_STATUS, B_XSTATE, B_SUMACC, B_SMOOTH, B_FILTER, B_SSUM};     // what a RESUME call reads back
    for (int rep = 0; rep < 400; ++rep) {
        hmcg_config cfg{};
        cfg.K = 2 + (int)(g() % 7); cfg.ldY = 2 + (int)(g() % 300); cfg.H = (int)(g() % 5); cfg.n_samples = (int)(g() % 4);
        cfg.window_base = g();
        const bool resume = coin();
        cfg.flags = resume ? HMCG_FLAG_RESUME : 0;
        const int n = 1 + (int)(g() % 40), W = n + (int)(g() % 20);
        std::vector<int32_t> perm((size_t)W);                      // a random subset of the caller's W rows in random order
        std::iota(perm.begin(), perm.end(), 0);
        std::shuffle(perm.begin(), perm.end(), g);
        const int32_t* idx = coin() ? perm.data() : nullptr;       // (or rows 0..n-1)
        // every caller array on or off; a non-null placeholder until the table says how wide its rows are
        char on;
        auto opt = [&]() -> void* { return coin() ? &on : nullptr; };
        hmcg_extras ex{};
        ex.struct_size = (int32_t)sizeof ex;
        HostArrays h{};
        h.Y = (const double*)&on; h.T = (const int32_t*)&on;
        h.yreal = (const double*)opt(); h.summary = (double*)opt(); h.status = (int32_t*)opt();
        ex.x_init = (const int32_t*)opt(); ex.x_final = (int32_t*)opt(); ex.pif_final = (double*)opt();
        ex.xstate = (uint8_t*)(resume ? &on : opt()); ex.sumacc = (double*)opt(); ex.window_ids = (const uint32_t*)opt();
        ex.sig_range = (const int32_t*)opt(); ex.save_range = (const int32_t*)opt(); ex.sigma_signal = (const double*)opt();
        ex.sigvals = (double*)opt(); ex.nsave_ld = (int32_t)(g() % 4); ex.end_pos = (const int32_t*)opt();
        ex.pi_smooth_mean = (double*)opt(); ex.pi_filter_mean = (double*)opt(); ex.corr = (double*)opt();
        ex.sample_summary = (double*)opt();
        h.ex = &ex;
        const bool need_ckpt = resume || ex.xstate || ex.sumacc || coin(), need_pif = coin();
        BufTable t = host_buffers(cfg, h, n, need_ckpt, need_pif, 1 + g() % 100);
        const size_t N = (size_t)n;

        // ---- layouts ----
        CHECK(t.resume == resume);
        CHECK(t.row[B_Y].doff == 0 && t.row[B_Y].poff == 0 && t.row[B_Y].bytes == 8 * (size_t)cfg.ldY);
        for (int i = 0; i < NBUF; ++i) {
            const Buf& a = t.row[i];
            CHECK((a.bytes == 0) == (a.doff == NO_OFF));
            if (!a.bytes) { CHECK(a.poff == NO_OFF); continue; }
            CHECK(a.doff % 256 == 0 && a.doff + N * a.bytes <= t.dev.total);
            if (a.staged()) CHECK(a.poff % 256 == 0 && a.poff + N * a.bytes <= t.pin.total);
            if (a.role == Role::in) CHECK(a.staged() && a.doff == a.poff && a.doff + N * a.bytes <= t.input_bytes);
            else CHECK(a.doff >= t.input_bytes && (!a.staged() || a.poff >= t.input_bytes));
            CHECK(a.zeroed == (a.doff >= t.zero_begin && a.doff < t.zero_end));
            if (a.host || (a.role == Role::inout && a.hook == Hook::resume_status)) CHECK(a.staged() || a.role == Role::in);
            for (int j = 0; j < i; ++j) {                          // no two buffers overlap, on either side
                const Buf& b = t.row[j];
                if (!b.bytes) continue;
                CHECK(a.doff + al(N * a.bytes) <= b.doff || b.doff + al(N * b.bytes) <= a.doff);
                if (a.staged() && b.staged()) CHECK(a.poff + al(N * a.bytes) <= b.poff || b.poff + al(N * b.bytes) <= a.poff);
            }
        }
        // the input block: Y, T, ids and the optional per-window inputs, the same bytes in both arenas
        size_t in_bytes = 0;
        for (const Buf& b : t.row) if (b.bytes && b.role == Role::in) in_bytes += al(N * b.bytes);
        CHECK(in_bytes == t.input_bytes && t.zero_begin == t.input_bytes);
        // the zeroed block: contiguous, exactly the outputs a skipped window never writes
        size_t z_bytes = 0;
        for (BufId id : zeroed_ids) { CHECK(t.row[id].zeroed); z_bytes += t.row[id].bytes ? al(N * t.row[id].bytes) : 0; }
        int nz = 0;
        for (const Buf& b : t.row) nz += b.zeroed ? 1 : 0;
        CHECK(nz == (int)(sizeof zeroed_ids / sizeof zeroed_ids[0]));
        CHECK(z_bytes == t.zero_end - t.zero_begin && t.row[B_STATUS].bytes == 4);
        for (int i = 0; i < NBUF; ++i) {
            bool r = false;
            for (BufId id : resume_ids) r |= id == i;
            CHECK((t.row[i].role == Role::inout) == r && (t.row[i].role == Role::in) == (i <= B_SIGMA));
            CHECK(t.row[i].ckpt == (i == B_STATUS || i == B_XSTATE || i == B_SUMACC));
        }
        // status and summary adjacent on both sides, returned in one copy
        const Buf &st = t.row[B_STATUS], &sm = t.row[B_SUMMARY];
        CHECK(st.staged() && st.returned());
        if (sm.bytes) CHECK(sm.same_copy && sm.doff == st.doff + al(4 * N) && sm.poff == st.poff + al(4 * N));
        for (const Buf& b : t.row) CHECK(!b.same_copy || &b == &sm);
        // the device slots: each row's pointer where the kernels look for it
        std::vector<char> dev(t.dev.total);
        const DevSlots ds = device_slots(t, dev.data());
        CHECK((const char*)ds.Y == dev.data() && (const char*)ds.ex.window_ids == dev.data() + t.row[B_WID].doff);
        CHECK((ds.ex.sumacc != nullptr) == need_ckpt && (ds.ex.corr != nullptr) == (ex.corr != nullptr) && (ds.mom != nullptr) == (ex.corr != nullptr));
        CHECK((ds.summary != nullptr) == (h.summary != nullptr) && (const char*)ds.status == dev.data() + st.doff);

        // ---- pack, then unpack: every caller row comes back, nothing else is touched ----
        std::vector<std::vector<char>> caller(NBUF), before(NBUF);
        for (int i = 0; i < NBUF; ++i) {
            Buf& b = t.row[i];
            if (!b.host) continue;
            caller[i].resize((size_t)W * b.bytes + 1);
            for (auto& c : caller[i]) c = (char)g();
            if (i == B_STATUS)                                    // caller status words without skip bits: they round-trip
                for (int w = 0; w < W; ++w) reinterpret_cast<int32_t*>(caller[i].data())[w] &= ~t.skip_mask;
            before[i] = caller[i];
            b.host = caller[i].data();
        }
        const unsigned char canary = 0xA5;
        std::vector<char> pin(t.pin.total + 64, (char)canary);
        const int split = (int)(g() % (unsigned)(n + 1));
        pack_rows(t, pin.data(), idx, 0, split);
        pack_rows(t, pin.data(), idx, split, n);
        std::vector<char> packed_mask(pin.size(), 0);
        for (int r = 0; r < NBUF; ++r) {
            const Buf& b = t.row[r];
            if (!b.sent(resume)) continue;
            for (int i = 0; i < n; ++i) {
                const size_t gr = idx ? (size_t)idx[i] : (size_t)i;
                const char* p = pin.data() + b.poff + (size_t)i * b.bytes;
                if (r == B_WID && !b.host) CHECK(*reinterpret_cast<const uint32_t*>(p) == cfg.window_base + (uint32_t)gr);
                else if (r == B_STATUS && !b.host) CHECK(*reinterpret_cast<const int32_t*>(p) == 0);
                else CHECK(memcmp(p, caller[r].data() + gr * b.bytes, b.bytes) == 0);
                memset(packed_mask.data() + (p - pin.data()), 1, b.bytes);
            }
        }
        for (size_t q = 0; q < pin.size(); ++q) CHECK(packed_mask[q] || (unsigned char)pin[q] == canary);   // nothing else written
        for (int r = 0; r < NBUF; ++r) if (t.row[r].role == Role::in && t.row[r].host) CHECK(caller[r] == before[r]);
        // the device's results: every returned row that was not sent gets fresh bytes, and a few windows are skipped
        for (int r = 0; r < NBUF; ++r) {
            const Buf& b = t.row[r];
            if (!b.returned() || b.sent(resume)) continue;
            for (size_t q = 0; q < N * b.bytes; ++q) pin[b.poff + q] = (char)g();
        }
        int32_t* pst = reinterpret_cast<int32_t*>(pin.data() + st.poff);
        for (int i = 0; i < n; ++i) pst[i] = (g() % 4 == 0) ? HMCG_ST_BAD_T : 0;
        std::vector<std::vector<char>> want = caller;
        for (int r = 0; r < NBUF; ++r) {
            const Buf& b = t.row[r];
            if (!b.returned() || !b.host) continue;
            for (int i = 0; i < n; ++i) {
                const size_t gr = idx ? (size_t)idx[i] : (size_t)i;
                char* dst = want[r].data() + gr * b.bytes;
                if (b.hook == Hook::zero_if_skipped && pst[i]) memset(dst, 0, b.bytes);
                else memcpy(dst, pin.data() + b.poff + (size_t)i * b.bytes, b.bytes);
            }
        }
        // (a RESUME call's inout rows come back as they went: the caller's own rows)
        if (resume)
            for (int r = 0; r < NBUF; ++r)
                if (r != B_STATUS && t.row[r].role == Role::inout && t.row[r].host) CHECK(want[r] == before[r]);
        unpack_rows(t, pin.data(), idx, n);
        for (int r = 0; r < NBUF; ++r) CHECK(caller[r] == want[r]);
    }
    return 0;
}

// ---- plan.hpp: make_plan on tables of the harness's own (null kernel pointers), against a brute-force restatement ----
static BigVariant g_forms[2][2][2][BIG_NK];       // [sig][smooth][stream][K - BIG_KMIN]
static const BigForm* const g_fake_big[2][2][2] = { { { &g_forms[0][0][0], &g_forms[0][0][1] }, { &g_forms[0][1][0], &g_forms[0][1][1] } },
                                                    { { &g_forms[1][0][0], &g_forms[1][0][1] }, { &g_forms[1][1][0], &g_forms[1][1][1] } } };

// one steps-per-thread class at 256 threads in the flavours of `mask` (1: P1, 2: P2, 4: H), as HMCG_V3 lays them out
static void add_class(std::vector<Variant>& out, int K, int L, bool sig, bool smooth, int pref_small, int pref_big, int mask = 7)
{
    if (mask & 1) out.push_back({K, L, 256, nullptr, sig, smooth, 0, 1, pref_small, pref_big});
    if (mask & 2) out.push_back({K, L, 256, nullptr, sig, smooth, 0, 2, pref_small, pref_big});
    if (mask & 4) out.push_back({K, L, 256, nullptr, sig, smooth, 4, 2, pref_small, pref_big});
}

struct FakeTable {
    std::vector<Variant> rows[2];                  // two groups
    VariantGroup grp[2];
    const VariantGroup* groups[2];
    KernelTables tab()
    {
        for (int g = 0; g < 2; ++g) { grp[g] = VariantGroup{rows[g].data(), (int)rows[g].size()}; groups[g] = &grp[g]; }
        return KernelTables{groups, 2, g_fake_big};
    }
};

static const char* const BADARG_SIG = "n_samples / sigma_signal / sigvals need extras.sig_range";

static int plan_rule_checks(const KernelTables& tab)
{
    char on;
    const auto lds = [](const BigVariant&) { return (size_t)0; };
    hmcg_config good{};
    good.struct_size = (int32_t)sizeof good; good.W = 4; good.K = 3; good.ldY = 300; good.max_T = 300; good.burnin = 5; good.nrun = 40; good.H = 2;
    hmcg_extras ex0{};
    ex0.struct_size = (int32_t)sizeof ex0;
    // the config and extras of a rule's smallest violation, and the message that goes with HMCG_E_BADARG
    struct Rule { const char* msg; std::function<void(hmcg_config&, hmcg_extras&)> breakit; };
    const Rule rules[] = {
        {"hmcg_extras.struct_size mismatch", [&](hmcg_config&, hmcg_extras& e) { e.struct_size = 8; }},
        {"HMCG_FLAG_RESUME needs extras.xstate", [&](hmcg_config& c, hmcg_extras&) { c.flags = HMCG_FLAG_RESUME; }},
        {BADARG_SIG, [&](hmcg_config& c, hmcg_extras&) { c.n_samples = 2; }},
        {BADARG_SIG, [&](hmcg_config&, hmcg_extras& e) { e.sigma_signal = (const double*)&on; }},
        {BADARG_SIG, [&](hmcg_config&, hmcg_extras& e) { e.sigvals = (double*)&on; e.nsave_ld = 1; }},
        {"blend_mask / end_pos need extras.sig_range", [&](hmcg_config& c, hmcg_extras&) { c.blend_mask = 1; }},
        {"blend_mask / end_pos need extras.sig_range", [&](hmcg_config&, hmcg_extras& e) { e.end_pos = (const int32_t*)&on; }},
        {"blend_mask has bits beyond H", [&](hmcg_config& c, hmcg_extras& e) { e.sig_range = (const int32_t*)&on; c.blend_mask = 4; }},
        {"blend_mask has bits beyond H", [&](hmcg_config& c, hmcg_extras& e) { e.sig_range = (const int32_t*)&on; c.blend_mask = -1; }},
        {"sigvals needs nsave_ld >= 1", [&](hmcg_config&, hmcg_extras& e) { e.sig_range = (const int32_t*)&on; e.sigvals = (double*)&on; }},
        {"sample_summary needs extras.sig_range (without the signal path it is `summary`)", [&](hmcg_config&, hmcg_extras& e) { e.sample_summary = (double*)&on; }},
        {"extras.corr: base runs only (no signal path), H >= 1 (the forecast column) and nrun >= 2", [&](hmcg_config&, hmcg_extras& e) { e.corr = (double*)&on; e.sig_range = (const int32_t*)&on; }},
        {"extras.corr: base runs only (no signal path), H >= 1 (the forecast column) and nrun >= 2", [&](hmcg_config& c, hmcg_extras& e) { e.corr = (double*)&on; c.H = 0; }},
        {"extras.corr: base runs only (no signal path), H >= 1 (the forecast column) and nrun >= 2", [&](hmcg_config& c, hmcg_extras& e) { e.corr = (double*)&on; c.nrun = 1; }},
        {"extras.corr needs the whole run in one call (no RESUME / sweep_base / sweep_count)", [&](hmcg_config& c, hmcg_extras& e) { e.corr = (double*)&on; c.flags = HMCG_FLAG_RESUME; e.xstate = (uint8_t*)&on; }},
        {"extras.corr needs the whole run in one call (no RESUME / sweep_base / sweep_count)", [&](hmcg_config& c, hmcg_extras& e) { e.corr = (double*)&on; c.sweep_base = 1; }},
        {"extras.corr needs the whole run in one call (no RESUME / sweep_base / sweep_count)", [&](hmcg_config& c, hmcg_extras& e) { e.corr = (double*)&on; c.sweep_count = 44; }},
        {"sweep_base beyond the run", [&](hmcg_config& c, hmcg_extras&) { c.sweep_base = 46; }},
    };
    Plan untouched, pl;
    char err[200] = "";
    CHECK(make_plan(tab, good, nullptr, 4, 256, 0, nullptr, PlanOverrides{}, lds, &pl, err, sizeof err) == 0 && err[0] == 0 && pl.v);
    CHECK(make_plan(tab, good, &ex0, 4, 256, 0, nullptr, PlanOverrides{}, lds, &pl, err, sizeof err) == 0 && err[0] == 0 && pl.v);
    for (const Rule& r : rules) {
        hmcg_config cfg = good;
        hmcg_extras ex = ex0;
        r.breakit(cfg, ex);
        pl = untouched;
        err[0] = 0;
        CHECK(make_plan(tab, cfg, &ex, 4, 256, 0, nullptr, PlanOverrides{}, lds, &pl, err, sizeof err) == HMCG_E_BADARG);
        CHECK(strcmp(err, r.msg) == 0);
        CHECK(pl.v == nullptr && pl.bv == nullptr);              // no plan comes back with an error
    }
    // (the rules that need no extras hold without them too; sweep_base AT the end of the run is a legal empty call)
    hmcg_config cfg = good;
    cfg.n_samples = 2;
    CHECK(make_plan(tab, cfg, nullptr, 4, 256, 0, nullptr, PlanOverrides{}, lds, &pl, err, sizeof err) == HMCG_E_BADARG && strcmp(err, BADARG_SIG) == 0);
    cfg = good;
    cfg.sweep_base = 45;
    CHECK(make_plan(tab, cfg, nullptr, 4, 256, 0, nullptr, PlanOverrides{}, lds, &pl, err, sizeof err) == 0 && pl.sched.sweep_begin == 45 && pl.sched.sweep_end == 45);
    return 0;
}

static int schedule_checks()
{
    std::mt19937_64 g(17);
    const int edge[] = {0, 1, 2, 3, 1000, 0x3fffffff, 0x7ffffffe, 0x7fffffff};
    auto pick = [&](long long most) {         // in [0, most], the small and the extreme values often
        const long long v = (g() & 1) ? (long long)edge[g() % 8] : (long long)(g() % (unsigned long long)(most + 1));
        return (int)std::min(v, most);
    };
    for (int rep = 0; rep < 20000; ++rep) {
        hmcg_config cfg{};
        cfg.n_samples = pick(rep % 3 ? 6 : 0x7fffffff);
        const long long ns = std::max(1, cfg.n_samples), per_most = 0x7fffffffLL / ns;    // validate(): n_samples * (burnin + nrun) <= 2^31 - 1
        cfg.burnin = pick(per_most);
        cfg.nrun = pick(per_most - cfg.burnin);
        cfg.sweep_base = pick(0x7fffffff);
        cfg.sweep_count = pick(0x7fffffff);
        const SweepSchedule s = sweep_schedule(cfg);
        const long long total = ns * ((long long)cfg.burnin + cfg.nrun), stop = (long long)cfg.sweep_base + cfg.sweep_count;
        const long long end = cfg.sweep_count > 0 && stop < total ? stop : total;
        CHECK(s.n_samples == ns && s.per_sample == std::max(1LL, (long long)cfg.burnin + cfg.nrun) && s.total_sweeps == total);
        CHECK(s.nd == ns * cfg.nrun && s.sweep_begin == cfg.sweep_base && s.sweep_end == end && s.final_launch == (end == total ? 1 : 0));
    }
    return 0;
}

static int plan_checks()
{
    for (int s = 0; s < 2; ++s) for (int m = 0; m < 2; ++m) for (int t = 0; t < 2; ++t)
        for (int k = 0; k < BIG_NK; ++k) g_forms[s][m][t][k] = BigVariant{BIG_KMIN + k, 256, nullptr};
    // A: the shape of the shipped K = 3 base path (eight classes in three flavours, rows at other block sizes), and a few more paths
    // B: gaps -- classes far apart, classes that lack flavours.  C: more classes than a call has bucket slots
    FakeTable tb[3];
    {
        const int LA[] = {1, 2, 4, 8, 3, 6, 12, 16}, prefA[][2] = {{H, P2}, {H, P1}, {H, P2}, {H, P2}, {H, P2}, {P2, P2}, {P1, P2}, {P1, H}};
        for (int i = 0; i < 8; ++i) add_class(tb[0].rows[i < 4 ? 0 : 1], 3, LA[i], false, false, prefA[i][0], prefA[i][1]);
        tb[0].rows[0].push_back({3, 2, 512, nullptr, false, false, 0, 1, P1, P1});
        tb[0].rows[0].push_back({3, 8, 128, nullptr, false, false, 0, 2, P2, P2});
        for (int L : {1, 2, 4}) add_class(tb[0].rows[1], 4, L, false, false, H, P2);
        for (int L : {1, 2, 4, 8}) add_class(tb[0].rows[1], 3, L, true, false, P2, H);
        for (int L : {1, 2, 4}) add_class(tb[0].rows[0], 3, L, false, true, H, H);
        for (int L : {2, 4}) add_class(tb[0].rows[0], 2, L, true, true, P1, P2);
        add_class(tb[1].rows[0], 3, 16, false, false, P1, P2, 4);          // H only
        add_class(tb[1].rows[0], 3, 1, false, false, H, P2);
        add_class(tb[1].rows[1], 3, 5, false, false, P1, H, 6);            // no P1
        add_class(tb[1].rows[1], 3, 9, false, false, H, P1, 3);            // no H
        tb[1].rows[0].push_back({3, 3, 256, nullptr, false, false, 0, 2, H, H});      // no H, and P2 ahead of P1
        tb[1].rows[0].push_back({3, 3, 256, nullptr, false, false, 0, 1, H, H});
        add_class(tb[1].rows[1], 2, 7, false, false, H, P2, 2);
        add_class(tb[1].rows[1], 2, 2, false, false, P2, P2);
        const int LC[] = {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16};
        for (int i = 0; i < 12; ++i) add_class(tb[2].rows[i % 2], 3, LC[i], false, false, i % 3, (i + 1) % 3);
        for (int L : {1, 2, 3, 4, 5, 6, 7, 8, 9, 10}) add_class(tb[2].rows[1], 4, L, false, true, H, P2);
    }
    if (plan_rule_checks(tb[0].tab())) return 1;
    if (schedule_checks()) return 1;

    std::mt19937 g(19);
    auto coin = [&]() { return (g() & 1) != 0; };
    auto one_in = [&](unsigned n) { return g() % n == 0; };
    char on;
    int seen_buckets = 0, seen_trunc = 0, seen_big = 0, seen_stream = 0, seen_unsupported = 0, seen_skipped_class = 0;
    for (int rep = 0; rep < 6000; ++rep) {
        FakeTable& ft = tb[rep % 3];
        const KernelTables tab = ft.tab();
        hmcg_config cfg{};
        cfg.struct_size = (int32_t)sizeof cfg;
        cfg.K = one_in(4) ? 2 + (int)(g() % 7) : (coin() ? 3 : 4);
        cfg.burnin = 3; cfg.nrun = 10; cfg.H = 1;
        const int maxT = one_in(5) ? 2 + (int)(g() % 9000) : 2 + (int)(g() % 4200);
        cfg.ldY = maxT + (int)(g() % 3);
        cfg.max_T = cfg.ldY == maxT && coin() ? 0 : maxT;                 // (0: ldY stands in)
        cfg.threads_per_window = one_in(6) ? (int)(g() % 4) * 128 + 128 : 0;
        hmcg_extras ex{};
        ex.struct_size = (int32_t)sizeof ex;
        const bool sig = one_in(4), smooth = one_in(4);
        if (sig) ex.sig_range = (const int32_t*)&on;
        if (smooth) (coin() ? ex.pi_smooth_mean : (coin() ? ex.pi_filter_mean : ex.pi_smooth_draws)) = (double*)&on;
        const int W = 1 + (int)(g() % 600), cu_count = 1 + (int)(g() % 512);
        // the windows: a few lengths of a ragged batch or every length of the range, and invalid ones among them
        std::vector<int32_t> T((size_t)W);
        const int span = coin() ? maxT : std::max(1, maxT / (1 + (int)(g() % 6))), few = one_in(3) ? 1 + (int)(g() % 3) : 0;
        int32_t some[3];
        for (int32_t& t : some) t = maxT - (int32_t)(g() % (unsigned)span);
        const int32_t bad[] = {INT32_MIN, INT32_MIN + 1, -7, 0, 1, maxT + 1, cfg.ldY + 300, INT32_MAX - 1, INT32_MAX};
        for (int32_t& t : T) t = one_in(9) ? bad[g() % 9] : (few ? some[g() % (unsigned)few] : maxT - (int32_t)(g() % (unsigned)span));
        std::vector<int32_t> perm((size_t)W);
        std::iota(perm.begin(), perm.end(), 0);
        std::shuffle(perm.begin(), perm.end(), g);
        const int n = 1 + (int)(g() % (unsigned)W);
        const bool host_entry = coin(), rows = host_entry && coin();       // host entry: lengths known; rows: a device's share of them
        const HostLengths hl{T.data(), rows ? perm.data() : nullptr, rows ? n : W};
        int minT = 0;
        if (host_entry) { for (int i = 0; i < hl.n; ++i) if (hl.at(i) >= 2 && (minT == 0 || hl.at(i) < minT)) minT = hl.at(i); }   // as HostCall::plan
        else minT = one_in(4) ? 0 : (one_in(8) ? maxT : 1 + (int)(g() % (unsigned)(maxT + 3)));                                     // the caller's hint
        PlanOverrides ov;
        const char* const fl_names[] = {"p1", "p2", "h"};
        const int force = one_in(4) ? (int)(g() % 3) : -1;
        if (force >= 0) ov.flavour = fl_names[force];
        const char* const bf_texts[] = {"h", "p2,h", "p1,p1,h,p2,p2,h,h,p1,p2,p2"};
        const int bf_codes[] = {H, -1, -1, -1, -1, -1, -1, -1, -1, -1, P2, H, -1, -1, -1, -1, -1, -1, -1, -1, P1, P1, H, P2, P2, H, H, P1, P2, P2};
        const int bf = one_in(4) ? (int)(g() % 3) : -1;
        if (bf >= 0) ov.bucket_flavours = bf_texts[bf];
        ov.force_big = one_in(12); ov.no_buckets = one_in(12); ov.force_stream = one_in(12); ov.stamps = one_in(12);
        // static LDS of the fake kernel: at, one above and around the largest that still fits
        const size_t dyn_want = (size_t)256 * (size_t)((maxT + 255) / 256) * 21 + 16, fit = 160 * 1024;
        const size_t stat = coin() ? (size_t)(g() % 60000) : (dyn_want <= fit ? fit - dyn_want + (coin() ? 1 : 0) : 0);
        int lds_calls = 0;
        const auto lds = [&](const BigVariant&) { ++lds_calls; return stat; };

        Plan pl;
        char err[200] = "";
        const int rc = make_plan(tab, cfg, &ex, hl.n, cu_count, minT, host_entry ? &hl : nullptr, ov, lds, &pl, err, sizeof err);
        const bool small_batch = hl.n <= cu_count;

        // ---- the restatement ----
        const int nt = cfg.threads_per_window > 0 ? cfg.threads_per_window : 256;
        std::vector<const Variant*> path;                       // the rows of this (K, block size, path), table order
        for (int gi = 0; gi < 2; ++gi) for (const Variant& v : ft.rows[gi]) if (v.K == cfg.K && v.NT == nt && v.sig == sig && v.smooth == smooth) path.push_back(&v);
        std::vector<int> classes;
        for (const Variant* v : path) classes.push_back(v->L);
        std::sort(classes.begin(), classes.end());
        classes.erase(std::unique(classes.begin(), classes.end()), classes.end());
        auto cover = [&](long long t) { for (int L : classes) if ((long long)nt * L >= t) return L; return 0; };     // 0: none
        // the row of class L the tie rule names: the wanted flavour, else P1, else the first
        auto row_of = [&](int L, int forced) {
            const Variant* first = nullptr; const Variant* p1 = nullptr;
            for (const Variant* v : path) {
                if (v->L != L) continue;
                if (flavour_of(*v) == (forced >= 0 ? forced : (small_batch ? v->pref_small : v->pref_big))) return v;
                if (!first) first = v;
                if (!p1 && flavour_of(*v) == P1) p1 = v;
            }
            return p1 ? p1 : first;
        };
        const int Lhi = cfg.K < 5 && !ov.force_big ? cover(maxT) : 0;
        CHECK(pl.sched.total_sweeps == 13 || rc != 0);
        if (Lhi == 0) {
            // the LDS-resident kernel: K >= 5, forced, or no register-resident row covers the longest window
            if (cfg.threads_per_window != 0 && cfg.threads_per_window != 256) {
                char want[200];
                snprintf(want, sizeof want, "no kernel for K=%d max_T=%d threads_per_window=%d", cfg.K, maxT, cfg.threads_per_window);
                CHECK(rc == HMCG_E_UNSUPPORTED && strcmp(err, want) == 0 && !pl.v && !pl.bv);
                ++seen_unsupported;
                continue;
            }
            const int bigL = (maxT + 255) / 256;
            const bool streams = dyn_want + stat > fit || ov.force_stream;
            CHECK(rc == 0 && err[0] == 0 && pl.v == nullptr && pl.nb == 0 && lds_calls == 1);
            CHECK(pl.bv == &g_forms[sig][smooth][streams][cfg.K - BIG_KMIN] && pl.bigL == bigL && pl.stream == streams && pl.dyn == (streams ? 16 : dyn_want));
            CHECK(pl.use_sig == sig && pl.use_smooth == smooth && pl.needs_pif() == smooth && pl.NT() == 256 && pl.L() == bigL && pl.NH() == 0);
            ++seen_big; seen_stream += streams;
            continue;
        }
        CHECK(rc == 0 && err[0] == 0 && pl.bv == nullptr && !pl.stream && pl.dyn == 0 && lds_calls == 0 && pl.use_sig == sig && pl.use_smooth == smooth && !pl.needs_pif());
        const int Llo = minT > 0 ? cover(minT) : 0;
        const bool cut = nt == 256 && cfg.threads_per_window == 0 && minT > 0 && minT < maxT && !ov.no_buckets && !ov.stamps && Llo < Lhi;
        std::vector<int> kept;                                   // the classes launched, longest first
        bool truncated = false;
        if (cut) {
            for (auto it = classes.rbegin(); it != classes.rend(); ++it) {
                if (*it > Lhi || *it < Llo) continue;
                bool any = !host_entry || *it == Lhi;
                for (int i = 0; host_entry && i < hl.n && !any; ++i) any = hl.at(i) >= 1 && cover(hl.at(i)) == *it;
                if (any) kept.push_back(*it); else ++seen_skipped_class;
            }
            truncated = (int)kept.size() > MAXBUCKET;
            kept.resize(std::min<size_t>(kept.size(), MAXBUCKET));
        }
        if (kept.size() <= 1) {
            // one launch, sized for the longest window (threads_per_window, no or equal minT, an override, or one class after all)
            CHECK(pl.nb == 0 && pl.v == row_of(Lhi, cut && bf >= 0 && bf_codes[10 * bf] >= 0 ? bf_codes[10 * bf] : force));
            CHECK(pl.NT() == nt && pl.L() == Lhi && pl.NH() == pl.v->NH && (long long)nt * Lhi >= maxT);
            continue;
        }
        ++seen_buckets; seen_trunc += truncated;
        const int nb = (int)kept.size();
        CHECK(pl.nb == nb && pl.v == pl.b[0].v);
        for (int j = 0; j < nb; ++j) {
            const int tok = bf >= 0 ? bf_codes[10 * bf + j] : -1;                     // per-bucket flavours: longest bucket first
            CHECK(pl.b[j].v == row_of(kept[(size_t)j], tok >= 0 ? tok : force) && pl.b[j].v->NT == 256);
        }
        // longest first, no gap, no overlap, and the two ends of int32_t
        CHECK(pl.b[0].t_hi == INT32_MAX && pl.b[nb - 1].t_lo == INT32_MIN);
        for (int j = 0; j < nb; ++j) CHECK(pl.b[j].t_lo <= pl.b[j].t_hi && (j == 0 || (pl.b[j].t_hi < pl.b[j - 1].t_lo && pl.b[j].t_hi + 1 == pl.b[j - 1].t_lo)));
        // where a length goes (the test of bucket_lists_kernel): exactly one bucket; a coverable one to the smallest kept class that covers it
        std::vector<int32_t> probe(T);
        probe.insert(probe.end(), std::begin(bad), std::end(bad));
        for (int L : classes) for (int d = -1; d <= 1; ++d) probe.push_back(256 * L + d);
        for (int i = 0; i < 40; ++i) probe.push_back((int32_t)g());
        for (int i = 0; i < 40; ++i) probe.push_back(2 + (int32_t)(g() % (unsigned)maxT));
        for (int32_t t : probe) {
            int hits = 0, at = -1;
            for (int j = 0; j < nb; ++j) if (t >= pl.b[j].t_lo && t <= pl.b[j].t_hi) { ++hits; at = j; }
            CHECK(hits == 1);
            int want = t > 256 * Lhi ? 0 : nb - 1;
            for (int j = 0; j < nb && t >= 1 && t <= 256 * Lhi; ++j) if (256 * kept[(size_t)j] >= t) want = j;        // (kept descends: the last that covers)
            CHECK(at == want);
            if (t >= 1 && t <= 256 * Lhi) CHECK(256 * pl.b[at].v->L >= t);             // also with more classes than slots
        }
        // the host entries' own windows run on the class their length selects among ALL classes (theirs is kept), slots permitting
        for (int i = 0; host_entry && !truncated && i < hl.n; ++i) {
            const int32_t t = hl.at(i);
            if (t < 2 || t > maxT) continue;
            for (int j = 0; j < nb; ++j) if (t >= pl.b[j].t_lo && t <= pl.b[j].t_hi) CHECK(pl.b[j].v->L == cover(t));
        }
    }
    // every branch above was taken
    CHECK(seen_buckets > 500 && seen_trunc > 10 && seen_big > 200 && seen_stream > 50 && seen_stream < seen_big && seen_unsupported > 10 && seen_skipped_class > 50);
    return 0;
}

static int csv_checks(const char* dir)
{
    char buf[64];
    const double xs[] = {0.0, 1.0, -1.0, 5.0, 0.1, 6.179999828338623, 24e-11, 46210605925778346e-23, 1e22, 1.7976931348623157e308,
                         4.9e-324, -2.5e-5, 123456.789, NAN, INFINITY, -INFINITY, 0.30000000000000004, 1e-4, 9.999e-5, 1e15, 1e16};
    for (double x : xs) {
        const int n = hmcg_format_float(x, buf);
        CHECK(n > 0 && n < 48 && (int)strlen(buf) == n);
        if (std::isfinite(x)) { double back = 0; CHECK(sscanf(buf, "%lf", &back) == 1 && back == x); }      // shortest round-trip text
    }
    const int K = 3, H = 2, W = 5;
    const int64_t nd = 700;
    const int32_t horizons[2] = {1, 12};
    std::mt19937_64 g(3);
    std::uniform_real_distribution<double> u(-10.0, 10.0);
    auto fill = [&](size_t n) { std::vector<double> v(n); for (auto& x : v) x = u(g); return v; };
    const auto mu = fill((size_t)W * K * nd), sig2 = fill((size_t)W * K * nd), pe = fill((size_t)W * K * nd), A = fill((size_t)W * K * K * nd),
               fc = fill((size_t)W * 2 * H * nd), sv = fill((size_t)W * 2 * 3);
    const char* dates[W] = {"1980-01-01", "1980-02-01", "1980-03-01", "1980-04-01", "1980-05-01"};
    CHECK(hmcg_save_results_csv(dir, W, dates, K, H, horizons, nd, mu.data(), sig2.data(), pe.data(), A.data(), fc.data(), nullptr, 0, 0, 0, 0, 4) == 0);
    // the signal layout: nd = n_samples * nrun, sigvals [W][n_samples][nsave_ld]
    const std::string d2 = std::string(dir) + "/sig";
    mkdir(d2.c_str(), 0755);
    CHECK(hmcg_save_results_csv(d2.c_str(), W, dates, K, H, horizons, nd, mu.data(), sig2.data(), pe.data(), A.data(), fc.data(), sv.data(), 2, 2, 3,
                                HMCG_CSV_LEGACY_TRANS_HEADER, 3) == 0);
    const char* names[3] = {"a", "b", "c"};
    const std::string p3 = std::string(dir) + "/table.csv";
    CHECK(hmcg_write_table_csv(p3.c_str(), "2000-01-01", 3, names, mu.data(), 100, nd, 5) == 0);
    CHECK(hmcg_write_table_csv("/nonexistent-dir/x.csv", "2000-01-01", 3, names, mu.data(), 100, nd, 5) != 0);
    FILE* f = fopen(p3.c_str(), "r");
    CHECK(f != nullptr);
    int lines = 0;
    for (int c; (c = fgetc(f)) != EOF;) lines += c == '\n';
    fclose(f);
    CHECK(lines == 101);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s <scratch dir>\n", argv[0]); return 2; }
    if (pool_checks()) return 1;
    if (partition_checks()) return 1;
    if (chunk_checks()) return 1;
    if (buffer_checks()) return 1;
    if (plan_checks()) return 1;
    if (csv_checks(argv[1])) return 1;
    printf("host harness ok\n");
    return 0;
}
