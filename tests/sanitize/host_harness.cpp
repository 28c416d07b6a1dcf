// Sanitizer harness for the host-side code of libhmcgibbs.so that needs no GPU (tests/test_sanitizers.py builds it with
// g++ -fsanitize=address,undefined and with -fsanitize=thread and runs it on the CPU):
//   * hmcg_hostutil::ScatterPool -- the helper threads of the host entry's scatter: start / run / stop / start again with a
//     job posted at once (the generation race of ADVICE r2), many jobs, jobs that write disjoint parts of one array;
//   * hmcg_hostutil::partition_windows, plan_chunks -- invariants on random shapes;
//   * hmcg_hostutil::host_buffers, pack_rows, unpack_rows -- the table of a host-entry call's per-window arrays on random
//     configurations: the arena layouts' invariants, and pack + unpack against the caller's rows;
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
#include "../../include/hmcg.h"

using namespace hmcg_hostutil;

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
    if (csv_checks(argv[1])) return 1;
    printf("host harness ok\n");
    return 0;
}
