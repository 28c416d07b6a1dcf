// hmcg.hip -- host side of libhmcgibbs.so (C ABI in include/hmcg.h).
//
// One lazily created context per HIP device: a compute stream, a copy stream, events and two grow-only
// workspaces (device memory and pinned host staging), so that a call costs no hipMalloc/hipFree once the
// workspaces have reached the size of the largest call.  Calls on one device are serialised by the context's
// mutex; different devices run concurrently (hmcg_estimate_batch_multi drives one host thread per device).
//
// The host entries stream results: a long chain is cut into a few chunks (big first, small last); chunk c's
// per-draw outputs go by SDMA into pinned staging and from there into the caller's arrays while chunk c+1
// samples.  The chain state between chunks travels through the same checkpoint block (xstate, sumacc) that
// HMCG_FLAG_RESUME exposes, so a chunked run is bit-identical to a single launch.
//
// What a call runs -- argument rules, kernel variant, length buckets, sweep range -- is decided in plan.hpp (plain C++, checked on the
// CPU); this unit hands it the tables and the diagnostic overrides (plan_call) and launches what comes back.
//
// No CPU compute path exists here: without a HIP device every compute entry returns HMCG_E_NODEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "gibbs_device.hpp"
#include "host_util.hpp"
#include "moments.hpp"
#include "plan.hpp"
#include "predictive.hpp"
#include "bias.hpp"
#include "mixmoments.hpp"
#include "density.hpp"
#include "autocorr.hpp"
#include "order.hpp"
#include "ergodic.hpp"
#include "fan.hpp"
#include "score.hpp"
#include "mixture_tile.hpp"

namespace {

thread_local char g_err[512] = "";

void set_err(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

// Diagnostic switches (fault injection, forced kernel forms, chunking overrides, virtual devices, trace) are armed by
// HMCG_DIAG=1, read ONCE when the library is first used: without it none of them is looked at -- no getenv on the call
// path, and a stray HMCG_* variable in a production environment changes nothing.  With it they are read per call, so a
// test process can switch them between calls.
bool diag_on()
{
    static const bool on = [] { const char* e = getenv("HMCG_DIAG"); return e && atoi(e) != 0; }();
    return on;
}
const char* diag_env(const char* name) { return diag_on() ? getenv(name) : nullptr; }

#define HIP_TRY(expr)                                                                  \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess) {                                                        \
            set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return (int)e_;                                                            \
        }                                                                              \
    } while (0)

// Grow-only allocation (device memory or pinned host memory).  Growing frees and reallocates: callers lay out a
// whole call before taking pointers, and nothing survives from one call to the next.
struct Arena {
    char* base = nullptr;
    size_t cap = 0;
    bool pinned = false;
    int ensure(size_t n)
    {
        if (n <= cap) return 0;
        release();
        const size_t want = std::max(n + n / 4, (size_t)1 << 20);
        hipError_t e = pinned ? hipHostMalloc((void**)&base, want, hipHostMallocDefault) : hipMalloc((void**)&base, want);
        if (e != hipSuccess) {
            base = nullptr;
            // retry with exactly what is needed before giving up
            e = pinned ? hipHostMalloc((void**)&base, n, hipHostMallocDefault) : hipMalloc((void**)&base, n);
            if (e != hipSuccess) { base = nullptr; cap = 0; return HMCG_E_NOMEM; }
            cap = n;
            return 0;
        }
        cap = want;
        return 0;
    }
    void release()
    {
        if (base) { if (pinned) (void)hipHostFree(base); else (void)hipFree(base); }
        base = nullptr; cap = 0;
    }
};

// Events that time launches, in pairs around each; released on every path out of a call.
struct Events {
    std::vector<hipEvent_t> ev;
    ~Events() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

using namespace hmcg_host;
using namespace hmcg_hostutil;
constexpr int RING = 3;            // chunk buffers in flight (device and pinned)

struct DeviceCtx {
    std::mutex mu;                 // serialises calls on this device
    bool ready = false;
    int device = -1;               // the id callers use (cfg->device, device_ids[])
    int phys = -1;                 // the HIP device behind it (== device unless HMCG_VIRTUAL_DEVICES is set)
    hipStream_t stream = nullptr, copy = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;          // kernel timing
    hipEvent_t ev_scr = nullptr;                      // device entry: last use of the shared arenas (scr, mom, ord) on any stream
    hipEvent_t evk[RING] = {}, evc[RING] = {};        // chunk pipeline: kernel done / copy done
    hipStream_t bstream[MAXBUCKET - 1] = {};          // length-bucketed dispatch: the shorter buckets' launches run beside the longest
    hipEvent_t ev_fork = nullptr, ev_join[MAXBUCKET - 1] = {};
    int cu_count = 0;
    Arena dev, pin;
    Arena mom;                     // device entry: the draw-moment tables behind extras.corr
    Arena scr;                     // device entry: the LDS-resident kernel's pdf scratch
    Arena ord;                     // device entry: the bucketed dispatch's window lists (bucket_lists_kernel)
    Arena pred;                    // device entry of the predictive CDFs: the slab sums
    Arena bias;                    // device entry of the uncertainty-bias moments: the slab sums and pivots
    Arena mix;                     // device entry of the predictive-mixture moments: the slab sums and pivots
    Arena dens;                    // device entry of the chain densities: the piece sums, pivots and range keys
    Arena acf;                     // device entry of the autocorrelations: the running lag sums, pivots and edge values
    Arena erg;                     // device entry of the ergodic moments: the slab sums and pivots
    Arena fan;                     // device entry of the predictive quantiles: the slab sums
    Arena score;                   // device entry of the predictive scores: the components, weights, slab sums and pair partials
    hmcg_hostutil::ScatterPool pool;              // host entries: helpers for the scatter into the caller's arrays
};
DeviceCtx g_ctx[HMCG_MAXDEV];
std::mutex g_init_mu;

// HMCG_VIRTUAL_DEVICES=n (diagnostics): the library offers n device ids, id i living on physical device i mod
// (physical count), each with its own context -- streams, arenas, scatter helpers.  It lets a one-GPU box execute the
// G > 1 branch of hmcg_estimate_batch_multi (worker threads, per-context workspaces, error aggregation) that otherwise
// needs a multi-GPU node.  0 / unset: ids are physical devices.
int virtual_devices()
{
    const char* e = diag_env("HMCG_VIRTUAL_DEVICES");          // (diagnostics only: read per call, so a test can switch it)
    const int n = e ? atoi(e) : 0;
    return n > 0 ? std::min(n, (int)HMCG_MAXDEV) : 0;
}

// Returns the (created on first use) context of `device`; the caller then locks ctx->mu and calls hipSetDevice(ctx->phys).
int get_context(int device, DeviceCtx** out)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_err("no HIP device available (libhmcgibbs has no CPU fallback)");
        return HMCG_E_NODEVICE;
    }
    const int nphys = n;
    if (virtual_devices() > 0) n = virtual_devices();
    if (device < 0 || device >= n || device >= HMCG_MAXDEV) {
        set_err("device %d out of range (count %d, at most %d)", device, n, HMCG_MAXDEV);
        return HMCG_E_BADARG;
    }
    DeviceCtx& c = g_ctx[device];
    std::lock_guard<std::mutex> lk(g_init_mu);
    if (!c.ready) {
        c.phys = device % nphys;
        HIP_TRY(hipSetDevice(c.phys));
        HIP_TRY(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&c.copy, hipStreamNonBlocking));
        HIP_TRY(hipEventCreate(&c.ev0));
        HIP_TRY(hipEventCreate(&c.ev1));
        HIP_TRY(hipEventCreateWithFlags(&c.ev_scr, hipEventDisableTiming));
        for (int i = 0; i < RING; ++i) {
            HIP_TRY(hipEventCreateWithFlags(&c.evk[i], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&c.evc[i], hipEventDisableTiming));
        }
        {
            // the shorter buckets' streams take the lowest priority: where blocks of two buckets compete for a CU, the
            // longer windows (the call's critical path) are placed first
            int lo = 0, hi = 0;
            HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
            for (int i = 0; i < MAXBUCKET - 1; ++i) {
                HIP_TRY(hipStreamCreateWithPriority(&c.bstream[i], hipStreamNonBlocking, lo));
                HIP_TRY(hipEventCreateWithFlags(&c.ev_join[i], hipEventDisableTiming));
            }
            HIP_TRY(hipEventCreateWithFlags(&c.ev_fork, hipEventDisableTiming));
        }
        HIP_TRY(hipDeviceGetAttribute(&c.cu_count, hipDeviceAttributeMultiprocessorCount, c.phys));
        c.pin.pinned = true;
        {
            // HMCG_SCATTER_THREADS: helper threads per device for the host-side scatter (default 3, 0 = the caller alone)
            int nw = 3;
            if (const char* e = getenv("HMCG_SCATTER_THREADS")) nw = atoi(e);
            const int hc = (int)std::thread::hardware_concurrency();
            if (hc > 0) nw = std::min(nw, std::max(0, hc - 1));
            c.pool.start(std::max(0, std::min(nw, 16)));
        }
        c.device = device;
        c.ready = true;
    }
    *out = &c;
    return 0;
}

void destroy_context(DeviceCtx& c)
{
    if (!c.ready) return;
    (void)hipSetDevice(c.phys);
    (void)hipStreamSynchronize(c.stream);        // nothing of ours may still be running when the streams go
    (void)hipStreamSynchronize(c.copy);
    (void)hipEventSynchronize(c.ev_scr);         // ... nor a device entry's work on a caller's stream: it may be using the arenas freed below
    (void)hipStreamDestroy(c.stream);
    (void)hipStreamDestroy(c.copy);
    (void)hipEventDestroy(c.ev0);
    (void)hipEventDestroy(c.ev1);
    (void)hipEventDestroy(c.ev_scr);
    for (int i = 0; i < RING; ++i) { (void)hipEventDestroy(c.evk[i]); (void)hipEventDestroy(c.evc[i]); }
    for (int i = 0; i < MAXBUCKET - 1; ++i) {
        (void)hipStreamSynchronize(c.bstream[i]);
        (void)hipStreamDestroy(c.bstream[i]);
        (void)hipEventDestroy(c.ev_join[i]);
        c.bstream[i] = nullptr;
    }
    (void)hipEventDestroy(c.ev_fork);
    c.dev.release();
    c.pin.release();
    c.mom.release();
    c.scr.release();
    c.ord.release();
    c.pred.release();
    c.bias.release();
    c.mix.release();
    c.dens.release();
    c.acf.release();
    c.erg.release();
    c.fan.release();
    c.score.release();
    c.pool.stop();
    c.stream = c.copy = nullptr;
    c.ready = false;
    c.device = c.phys = -1;
}

// Argument rules of hmcg_config; 0 or HMCG_E_BADARG with the reason in msg (as the check_* of the statistics).
int validate(const hmcg_config* cfg, char* msg, size_t nmsg)
{
    if (!cfg) { snprintf(msg, nmsg, "cfg is NULL"); return HMCG_E_BADARG; }
    if (cfg->struct_size != (int32_t)sizeof(hmcg_config)) {
        snprintf(msg, nmsg, "hmcg_config.struct_size %d != %d", cfg->struct_size, (int)sizeof(hmcg_config));
        return HMCG_E_BADARG;
    }
    if (cfg->W < 1 || cfg->K < 2 || cfg->K > HMCG_MAXK || cfg->ldY < 2 || cfg->burnin < 0 || cfg->nrun < 0 ||
        cfg->H < 0 || cfg->H > HMCG_MAXH || cfg->max_T < 0 || cfg->max_T > cfg->ldY || cfg->sweep_base < 0 || cfg->sweep_count < 0 || cfg->n_samples < 0 || cfg->kappa < 0.0 || cfg->min_T < 0) {
        snprintf(msg, nmsg, "bad hmcg_config (W=%d K=%d ldY=%d max_T=%d burnin=%d nrun=%d H=%d)", cfg->W, cfg->K, cfg->ldY,
                cfg->max_T, cfg->burnin, cfg->nrun, cfg->H);
        return HMCG_E_BADARG;
    }
    for (int h = 0; h < cfg->H; ++h)
        if (cfg->horizons[h] < 0) { snprintf(msg, nmsg, "negative horizon"); return HMCG_E_BADARG; }
    if ((long long)(cfg->n_samples > 1 ? cfg->n_samples : 1) * ((long long)cfg->burnin + cfg->nrun) > 0x7fffffffLL) {
        snprintf(msg, nmsg, "n_samples * (burnin + nrun) exceeds 2^31 - 1 sweeps");
        return HMCG_E_BADARG;
    }
    return 0;
}

// Static LDS of a kernel instantiation, asked of the runtime once per function (plan_call and fill_timing sit on the call path).
size_t static_lds_bytes(const void* fn, size_t fallback)
{
    static std::mutex mu;
    static std::vector<std::pair<const void*, size_t>> cache;
    std::lock_guard<std::mutex> lk(mu);
    for (const auto& e : cache) if (e.first == fn) return e.second;
    hipFuncAttributes fa{};
    if (hipFuncGetAttributes(&fa, fn) != hipSuccess) return fallback;      // (not cached: asked again next time)
    cache.emplace_back(fn, fa.sharedSizeBytes);
    return fa.sharedSizeBytes;
}

// What runs: make_plan (plan.hpp) on the library's own tables.  The ONE place that reads the diagnostic switches of the kernel
// choice, and where the stamps build says that it is one.
int plan_call(const hmcg_config* cfg, const hmcg_extras* ex, int W, int cu_count, int minT, const HostLengths* hl, Plan* plan)
{
    static const VariantGroup* const groups[] = { &g_group_k2, &g_group_k3, &g_group_mid, &g_group_k3_l16, &g_group_k4, &g_group_sig, &g_group_smooth, &g_group_sigsmooth };
    const KernelTables tab{groups, (int)(sizeof groups / sizeof groups[0]), g_big};
    PlanOverrides ov;
    ov.flavour = diag_env("HMCG_FLAVOUR");
    ov.bucket_flavours = diag_env("HMCG_BUCKET_FLAVOURS");
    ov.force_big = diag_env("HMCG_FORCE_BIG") != nullptr;
    ov.no_buckets = diag_env("HMCG_NO_BUCKETS") != nullptr;
    ov.force_stream = diag_env("HMCG_FORCE_STREAM") != nullptr;
#if defined(HMCG_STAMPS) || defined(HMCG_BARRIER_STAMPS)
    ov.stamps = true;
#endif
    const auto static_lds = [](const BigVariant& bv) { return static_lds_bytes(reinterpret_cast<const void*>(bv.fn), 48 * 1024); };
    char msg[160];
    const int rc = make_plan(tab, *cfg, ex, W, cu_count, minT, hl, ov, static_lds, plan, msg, sizeof msg);
    if (rc) set_err("%s", msg);
    return rc;
}

// The LDS-resident kernel's device scratch: per-step pdfs handed from the product phase to the replay, [W][L][ceil(K/2)][NT][2] doubles
size_t scratch_bytes(const Plan& pl, int W, int K) { return pl.bv ? sizeof(double) * (size_t)W * (size_t)pl.bigL * (size_t)(2 * hmcg::big_scratch_pairs(K)) * (size_t)pl.bv->NT : 0; }
// streaming form: per window the observations, uniforms, state maps and states of its NT * L steps
size_t slab_bytes(const Plan& pl) { return pl.stream ? hmcg::stream_slab_bytes((size_t)pl.bv->NT * (size_t)pl.bigL) : 0; }
size_t stream_bytes(const Plan& pl, int W) { return slab_bytes(pl) * (size_t)W; }

// Kernel parameters common to every launch of a call; per-launch fields (sweep range, resume, output window) are
// filled by the caller.  All pointers are device pointers.
hmcg::KernelParams base_params(const hmcg_config* cfg, int W, const double* dY, const int32_t* dT, const double* dyreal,
                               int32_t* dstatus, const hmcg_extras* dex, const Plan& pl)
{
    hmcg::KernelParams p{};
    p.Y = dY; p.T = dT; p.yreal = dyreal;
    p.ldY = cfg->ldY; p.W = W; p.H = cfg->H;
    p.per_sample = pl.sched.per_sample;
    p.burnin_s = cfg->burnin; p.nrun_s = cfg->nrun; p.n_samples = pl.sched.n_samples; p.nd = pl.sched.nd;
    p.kappa = cfg->kappa;
    for (int h = 0; h < HMCG_MAXH; ++h) p.horizons[h] = h < cfg->H ? cfg->horizons[h] : 0;
    p.seed_lo = (uint32_t)cfg->seed; p.seed_hi = (uint32_t)(cfg->seed >> 32); p.window_base = cfg->window_base;
    p.alpha = cfg->alpha > 0.0 ? cfg->alpha : 1.0;
    p.nu = cfg->nu > 0.0 ? cfg->nu : 1.0;
    p.status = dstatus;
    if (dex) {
        p.pi_smooth_mean = dex->pi_smooth_mean; p.pi_filter_mean = dex->pi_filter_mean; p.pi_smooth_draws = dex->pi_smooth_draws;
        p.sig_range = dex->sig_range; p.save_range = dex->save_range; p.sigma_signal = dex->sigma_signal;
        p.sigvals = dex->sigvals; p.nsave_ld = dex->nsave_ld;
        p.x_init = dex->x_init; p.x_final = dex->x_final; p.pif_final = dex->pif_final; p.xstate = dex->xstate;
        p.sumacc = dex->sumacc; p.window_ids = dex->window_ids;
        if (pl.use_sig) { p.end_pos = dex->end_pos; p.blend_mask = cfg->blend_mask; p.sample_summary = dex->sample_summary; }
    }
    return p;
}

// ---- the bucketed dispatch's window lists (KernelParams::order): per bucket a block of 4 + W words (n, t_lo, t_hi, -, ids),
// then two words: the number of class changes between neighbouring windows, and the ticket of the last block ----
constexpr int ORD_HDR = 4;
struct BucketRanges { int nb; int compact; int lo[MAXBUCKET], hi[MAXBUCKET]; };
__global__ void bucket_lists_kernel(const int32_t* T, int W, BucketRanges r, int32_t* ord)
{
    const size_t stride = (size_t)W + ORD_HDR;
    int32_t* meta = ord + (size_t)MAXBUCKET * stride;
    const int w = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (w < W) {
        auto bucket_of = [&](int t) { int k = 0; for (int b = 0; b < r.nb; ++b) if (t >= r.lo[b] && t <= r.hi[b]) k = b; return k; };
        const int mine = bucket_of(T[w]);           // exactly one bucket: the first reaches INT32_MAX, the last starts at INT32_MIN
        int32_t* list = ord + (size_t)mine * stride;
        const int pos = atomicAdd(&list[0], 1);
        list[ORD_HDR + pos] = w;
        if (w > 0 && bucket_of(T[w - 1]) != mine) atomicAdd(&meta[0], 1);
    }
    // the last block to get here closes the lists: ranges into the headers; and when every class is one run of the caller's
    // windows (changes == non-empty classes - 1) there is nothing to compact -- n = -1, block b keeps window b (1.7 % faster
    // than the compacted launches on the sorted production batch, measured).  r.compact == 0 (diagnostics): never compact.
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0 && atomicAdd(&meta[1], 1) == (int)gridDim.x - 1) {
        __threadfence();
        int runs = 0;
        for (int b = 0; b < r.nb; ++b) runs += atomicAdd(&ord[(size_t)b * stride], 0) > 0 ? 1 : 0;
        const bool sorted = atomicAdd(&meta[0], 0) == runs - 1 || !r.compact;
        for (int b = 0; b < r.nb; ++b) {
            int32_t* list = ord + (size_t)b * stride;
            if (sorted) list[0] = -1;
            list[1] = r.lo[b]; list[2] = r.hi[b];
        }
    }
}
size_t bucket_list_bytes(int W) { return sizeof(int32_t) * ((size_t)MAXBUCKET * ((size_t)W + ORD_HDR) + 2); }
// Enqueues the list construction on `stream` (T on the device): one memset, one kernel.  The order inside a list is whatever
// the atomics give: every window's result is independent of the block that runs it.
int build_bucket_lists(const Plan& pl, const int32_t* dT, int W, int32_t* ord, hipStream_t stream)
{
    BucketRanges r{};
    r.nb = pl.nb;
    r.compact = diag_env("HMCG_NO_BUCKET_LISTS") ? 0 : 1;
    for (int b = 0; b < pl.nb; ++b) { r.lo[b] = pl.b[b].t_lo; r.hi[b] = pl.b[b].t_hi; }
    HIP_TRY(hipMemsetAsync(ord, 0, bucket_list_bytes(W), stream));
    hipLaunchKernelGGL(bucket_lists_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, stream, dT, W, r, ord);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ord: the lists built by build_bucket_lists for this plan and these windows (bucketed plans), or null
int launch_kernel(DeviceCtx& c, const Plan& pl, const hmcg::KernelParams& p, hipStream_t stream, const int32_t* ord)
{
    if (pl.nb > 1) {
        // fork: every bucket's launch waits for what precedes this call on `stream`; the longest bucket runs on `stream`
        // itself, the others on the context's bucket streams; join: `stream` waits for all of them
        HIP_TRY(hipEventRecord(c.ev_fork, stream));
        for (int b = 0; b < pl.nb; ++b) {
            hipStream_t bs = b == 0 ? stream : c.bstream[b - 1];
            if (b > 0) HIP_TRY(hipStreamWaitEvent(bs, c.ev_fork, 0));
            hmcg::KernelParams q = p;
            q.order = ord + (size_t)b * ((size_t)p.W + ORD_HDR);
            const Variant* v = pl.b[b].v;
            hipLaunchKernelGGL(v->fn, dim3((unsigned)p.W), dim3((unsigned)(v->NT + 64 * v->NH)), 0, bs, q);
            HIP_TRY(hipGetLastError());
            if (b > 0) HIP_TRY(hipEventRecord(c.ev_join[b - 1], bs));
        }
        for (int b = 1; b < pl.nb; ++b) HIP_TRY(hipStreamWaitEvent(stream, c.ev_join[b - 1], 0));
        return 0;
    }
    if (pl.v) hipLaunchKernelGGL(pl.v->fn, dim3((unsigned)p.W), dim3((unsigned)(pl.v->NT + 64 * pl.v->NH)), 0, stream, p);
    else hipLaunchKernelGGL(pl.bv->fn, dim3((unsigned)p.W), dim3((unsigned)pl.bv->NT), pl.dyn, stream, p, pl.bigL);
    HIP_TRY(hipGetLastError());
    return 0;
}

void fill_timing(hmcg_timing* t, const Plan& pl, const DeviceCtx& c, double kernel_ms, int launches, double call_ms, int windows)
{
    if (!t) return;
    t->kernel_ms = kernel_ms;
    t->launches = launches;
    t->threads_per_window = pl.NT();
    t->steps_per_thread = pl.L();
    t->helper_waves = pl.NH();
    t->device = c.device;
    t->call_ms = call_ms;
    t->windows = windows;
    t->occupancy = pl.v ? pl.v->occ : 0;
    t->buckets = pl.nb > 1 ? pl.nb : 1;
    t->streaming = pl.stream ? 1 : 0;
    t->lds_bytes = (int32_t)(static_lds_bytes(pl.fptr(), 0) + pl.dyn);
}

#ifdef HMCG_STAMPS
int print_stamps(const hmcg::KernelParams& p, const Plan& pl, unsigned long long* ddbg, size_t ndbg, hipStream_t stream)
{
    static const char* names[HMCG_NSTAMP] = {"Ba wait", "param draws | shadow jobs", "Bb wait", "theta+ux+pdfs", "local product",
        "wave scan", "Bc wait", "prefix+replay+last", "Bd wait", "maps+compose", "map scan", "Be wait", "apply", "publish sums", "  (shadow: outputs)", "  (shadow: prep)", "  (param: counts+row sums)", "  (param: shapes)", "  (param: gamma)", "  (stats: counts)", "Ba2 wait", "param finish | half trips", "  (shadow: ux ahead)"};
    const int nwv = pl.NT() / 64 + pl.NH();
    std::vector<unsigned long long> h(ndbg);
    HIP_TRY(hipStreamSynchronize(stream));
    // HMCG_STAMPS_AFTER=n: stay silent for the first n launches (tools/stamps.py warms the chip up for >= 2 s first)
    static int launches_seen = 0;
    static const int print_after = diag_env("HMCG_STAMPS_AFTER") ? atoi(diag_env("HMCG_STAMPS_AFTER")) : 0;
    if (launches_seen++ < print_after) return 0;
    HIP_TRY(hipMemcpy(h.data(), ddbg, ndbg * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    const int nsw = p.sweep_end - p.sweep_begin;
    {
        // in-kernel clock of every wave: d(s_memtime) / d(s_memrealtime) * 100 MHz around the sweep loop
        std::vector<double> clk;
        double ticks = 0;
        for (int w = 0; w < p.W; ++w)
            for (int wv = 0; wv < nwv; ++wv) {
                const unsigned long long* o = &h[((size_t)w * nwv + wv) * HMCG_NSTAMP_ALL];
                if (o[HMCG_NSTAMP + 1]) { clk.push_back(100.0 * (double)o[HMCG_NSTAMP] / (double)o[HMCG_NSTAMP + 1]); ticks += (double)o[HMCG_NSTAMP]; }
            }
        std::sort(clk.begin(), clk.end());
        if (!clk.empty())
            fprintf(stderr, "[clock] launch %d: in-kernel clock MHz min %.0f median %.0f max %.0f (s_memtime / s_memrealtime x 100 MHz); "
                            "%.0f ticks per sweep (mean over waves)\n", launches_seen - 1, clk.front(), clk[clk.size() / 2], clk.back(),
                    ticks / (double)clk.size() / (nsw > 0 ? nsw : 1));
    }
    fprintf(stderr, "[stamps] K=%d L=%d NT=%d W=%d sweeps=%d: mean cycles per sweep by wave (s_memtime ticks)\n",
            pl.v ? pl.v->K : pl.bv->K, pl.L(), pl.NT(), p.W, nsw);
    fprintf(stderr, "%-24s", "phase");
    for (int wv = 0; wv < nwv; ++wv) fprintf(stderr, "   wave%-2d", wv);
    fprintf(stderr, "\n");
    std::vector<double> tot(nwv, 0.0);
    for (int i = 0; i < HMCG_NSTAMP; ++i) {
        fprintf(stderr, "%-24s", names[i]);
        for (int wv = 0; wv < nwv; ++wv) {
            double acc = 0;
            for (int w = 0; w < p.W; ++w) acc += (double)h[((size_t)w * nwv + wv) * HMCG_NSTAMP_ALL + i];
            acc /= (double)p.W * (nsw > 0 ? nsw : 1);
            tot[wv] += acc;
            fprintf(stderr, " %8.0f", acc);
        }
        fprintf(stderr, "\n");
    }
    fprintf(stderr, "%-24s", "total");
    for (int wv = 0; wv < nwv; ++wv) fprintf(stderr, " %8.0f", tot[wv]);
    fprintf(stderr, "\n");
    return 0;
}
#endif

#ifdef HMCG_BARRIER_STAMPS
// The barrier-arrival build's table: per wave and sweep barrier the mean ticks from the previous release to the arrival (work)
// and from the arrival to the release (wait).  Same switches and the same [clock] line as the phase-stamped build.
int print_stamps(const hmcg::KernelParams& p, const Plan& pl, unsigned long long* ddbg, size_t ndbg, hipStream_t stream)
{
    static const char* names[HMCG_NBAR] = {"Ba", "Ba2", "Bb", "Bc", "Bd", "Be"};
    HIP_TRY(hipStreamSynchronize(stream));
    static int launches_seen = 0;
    static const int print_after = diag_env("HMCG_STAMPS_AFTER") ? atoi(diag_env("HMCG_STAMPS_AFTER")) : 0;
    if (launches_seen++ < print_after) return 0;
    if (!pl.v) return 0;                        // the LDS-resident kernels carry no barrier stamps
    const int nwv = pl.NT() / 64 + pl.NH();
    std::vector<unsigned long long> h(ndbg);
    HIP_TRY(hipMemcpy(h.data(), ddbg, ndbg * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    const int nsw = p.sweep_end - p.sweep_begin;
    const double per = (double)p.W * (nsw > 0 ? nsw : 1);
    {
        std::vector<double> clk;
        double ticks = 0;
        for (int w = 0; w < p.W; ++w)
            for (int wv = 0; wv < nwv; ++wv) {
                const unsigned long long* o = &h[((size_t)w * nwv + wv) * HMCG_NSTAMP_ALL];
                if (o[2 * HMCG_NBAR + 1]) { clk.push_back(100.0 * (double)o[2 * HMCG_NBAR] / (double)o[2 * HMCG_NBAR + 1]); ticks += (double)o[2 * HMCG_NBAR]; }
            }
        std::sort(clk.begin(), clk.end());
        if (!clk.empty())
            fprintf(stderr, "[clock] launch %d: in-kernel clock MHz min %.0f median %.0f max %.0f (s_memtime / s_memrealtime x 100 MHz); "
                            "%.0f ticks per sweep (mean over waves)\n", launches_seen - 1, clk.front(), clk[clk.size() / 2], clk.back(),
                    ticks / (double)clk.size() / (nsw > 0 ? nsw : 1));
    }
    fprintf(stderr, "[barrier stamps] K=%d L=%d NT=%d W=%d sweeps=%d: mean ticks per sweep by wave (s_memtime)\n",
            pl.v->K, pl.L(), pl.NT(), p.W, nsw);
    fprintf(stderr, "%-24s", "barrier");
    for (int wv = 0; wv < nwv; ++wv) fprintf(stderr, "   wave%-2d", wv);
    fprintf(stderr, "\n");
    std::vector<double> tot(nwv, 0.0);
    for (int i = 0; i < 2 * HMCG_NBAR; ++i) {
        const int b = i / 2, slot = (i & 1) ? HMCG_NBAR + b : b;      // work to Ba, wait at Ba, work to Ba2, ...
        char label[32];
        snprintf(label, sizeof label, (i & 1) ? "%s wait" : "work -> %s", names[b]);
        fprintf(stderr, "%-24s", label);
        for (int wv = 0; wv < nwv; ++wv) {
            double acc = 0;
            for (int w = 0; w < p.W; ++w) acc += (double)h[((size_t)w * nwv + wv) * HMCG_NSTAMP_ALL + slot];
            acc /= per;
            tot[wv] += acc;
            fprintf(stderr, " %8.0f", acc);
        }
        fprintf(stderr, "\n");
    }
    fprintf(stderr, "%-24s", "total");
    for (int wv = 0; wv < nwv; ++wv) fprintf(stderr, " %8.0f", tot[wv]);
    fprintf(stderr, "\n");
    return 0;
}
#endif

// ---- device-resident entry: one launch over caller-owned HBM buffers -----------------------------------------

// Grows one of the device entry's context-owned arenas (scr, mom, ord).  An enqueue-only call on any stream may still be
// using the old buffer: growing waits for its last use (ev_scr) before the old one is freed.
int grow_shared(DeviceCtx& c, Arena& a, size_t bytes)
{
    if (a.cap >= bytes) return 0;
    HIP_TRY(hipEventSynchronize(c.ev_scr));
    if (a.ensure(bytes)) { set_err("workspace allocation failed (%zu B device)", bytes); return HMCG_E_NOMEM; }
    return 0;
}

int launch_device(DeviceCtx& c, const hmcg_config* cfg, const double* dY, const int32_t* dT, const double* dyreal, double* dmu,
                  double* dsig2, double* dA, double* dpi_end, double* dfcast, double* dsummary, int32_t* dstatus,
                  const hmcg_extras* ex, hipStream_t stream, hmcg_timing* timing)
{
    if (!dY || !dT || !dstatus) { set_err("Y, T and status are required"); return HMCG_E_BADARG; }
    Plan pl;
    int rc = plan_call(cfg, ex, cfg->W, c.cu_count, cfg->min_T, nullptr, &pl);
    if (rc) return rc;
    if (pl.needs_pif() && !(ex && ex->pif_final)) {
        set_err("pi_smooth_mean / pi_filter_mean for K >= 5 or windows beyond the register-resident kernels need extras.pif_final "
                "([W][ldY][K]: the running sweep's filtered probabilities pass through it)");
        return HMCG_E_BADARG;
    }
    if (ex && ex->corr && (!dmu || !dsig2 || !dA || !dpi_end || !dfcast)) {
        set_err("extras.corr on the device entry needs all five per-draw outputs");
        return HMCG_E_BADARG;
    }
    const bool resume = (cfg->flags & HMCG_FLAG_RESUME) != 0;
    hmcg::KernelParams p = base_params(cfg, cfg->W, dY, dT, dyreal, dstatus, ex, pl);
    p.sweep_begin = pl.sched.sweep_begin; p.sweep_end = pl.sched.sweep_end; p.final_launch = pl.sched.final_launch;
    p.resume = resume ? 1 : 0;
    p.mu = dmu; p.sig2 = dsig2; p.A = dA; p.pi_end = dpi_end; p.fcast = dfcast; p.summary = dsummary;
    p.nd_ld = p.nd; p.draw_off = 0;

    if (!resume) HIP_TRY(hipMemsetAsync(dstatus, 0, sizeof(int32_t) * (size_t)cfg->W, stream));
    // The pdf scratch and the moment tables belong to the device context, not to the call: an enqueue-only call on another
    // stream may still be using them, so this launch is ordered behind their last use.
    const bool use_lists = pl.nb > 1;
    const bool uses_scratch = pl.bv != nullptr || (ex && ex->corr) || use_lists;
    if (uses_scratch) HIP_TRY(hipStreamWaitEvent(stream, c.ev_scr, 0));
    int32_t* ord = nullptr;
    if (use_lists) {
        if ((rc = grow_shared(c, c.ord, bucket_list_bytes(cfg->W)))) return rc;
        ord = reinterpret_cast<int32_t*>(c.ord.base);
    }
    if (pl.bv) {
        HIP_TRY(hipFuncSetAttribute(pl.fptr(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.dyn));
        const size_t fbytes = (scratch_bytes(pl, cfg->W, cfg->K) + 255) & ~(size_t)255;
        const size_t sbytes = fbytes + stream_bytes(pl, cfg->W);
        if ((rc = grow_shared(c, c.scr, sbytes))) return rc;
        p.fscr = reinterpret_cast<double*>(c.scr.base);
        if (pl.stream) { p.sscr = reinterpret_cast<uint8_t*>(c.scr.base + fbytes); p.stream_stride = (int64_t)slab_bytes(pl); }
    }
    if (timing) HIP_TRY(hipEventRecord(c.ev0, stream));
#if defined(HMCG_STAMPS) || defined(HMCG_BARRIER_STAMPS)
    const size_t ndbg = (size_t)cfg->W * (pl.NT() / 64 + pl.NH()) * HMCG_NSTAMP_ALL;
    unsigned long long* ddbg = nullptr;
    HIP_TRY(hipMalloc((void**)&ddbg, ndbg * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(ddbg, 0, ndbg * sizeof(unsigned long long), stream));
    p.dbg = ddbg;
#endif
    if (ord) { rc = build_bucket_lists(pl, dT, cfg->W, ord, stream); if (rc) return rc; }
    rc = launch_kernel(c, pl, p, stream, ord);
    if (rc) return rc;
    if (ex && ex->corr) {
        // correlations of the rounded draws (calccorr): one pass over the draw arrays while they are in HBM
        const size_t mbytes = sizeof(double) * (size_t)cfg->W * hmcg_host::moments_stride(cfg->K);
        if ((rc = grow_shared(c, c.mom, mbytes))) return rc;
        hmcg_host::MomentsArgs ma{dmu, dsig2, dpi_end, dA, dfcast, reinterpret_cast<double*>(c.mom.base), cfg->nrun, cfg->nrun, cfg->W, cfg->K, cfg->H, true};
        HIP_TRY(hmcg_host::launch_moments(ma, stream));
        HIP_TRY(hmcg_host::launch_corr_finalize(reinterpret_cast<double*>(c.mom.base), ex->corr, cfg->W, cfg->K, stream));
    }
    if (uses_scratch) HIP_TRY(hipEventRecord(c.ev_scr, stream));
#if defined(HMCG_STAMPS) || defined(HMCG_BARRIER_STAMPS)
    rc = print_stamps(p, pl, ddbg, ndbg, stream);
    (void)hipFree(ddbg);
    if (rc) return rc;
#endif
    if (timing) {
        HIP_TRY(hipEventRecord(c.ev1, stream));
        HIP_TRY(hipEventSynchronize(c.ev1));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c.ev0, c.ev1));
        fill_timing(timing, pl, c, ms, 1, 0.0, cfg->W);
    }
    return 0;
}

// ---- host entry on one device --------------------------------------------------------------------------------

// One host-entry call on one device, step by step: plan() picks the kernel and cuts the chain into chunks, lay_out() places
// every buffer in the two arenas, stage_inputs() packs and sends what the kernels read, run_chunks() runs the chain and
// scatters each chunk's draws into the caller's arrays, collect_outputs() hands back the rest.  The per-window arrays are
// rows of one table (host_util.hpp, host_buffers); the per-draw chunk columns are laid out here.
// Caller holds c.mu and has made c.device current.
struct HostCall {
    DeviceCtx& c;
    const hmcg_config* cfg;
    const int32_t* idx;            // the call's windows: rows idx[0..n) of the caller's arrays (nullptr: rows 0..n-1)
    int n;
    const HostArrays& h;
    hmcg_timing* timing;
    std::chrono::steady_clock::time_point t_call = std::chrono::steady_clock::now();
    std::vector<std::pair<const char*, double>> trace;

    Plan pl;
    // per-draw output columns of one window, in the order they sit in a chunk buffer
    struct Col { double* host; size_t ncol; size_t off; };
    Col cols[6] = {};
    size_t ncols = 0;
    bool stream_draws = false, copy_out = false, want_corr = false;
    long long nd_total = 0;        // kept draws per window over the whole run
    std::vector<Chunk> chunks;

    BufTable bt{};
    char* D = nullptr;
    char* P = nullptr;
    size_t o_dchunk[RING] = {}, o_pchunk[RING] = {}, o_pst0 = 0;
    int32_t* dord = nullptr;       // the bucketed dispatch's window lists
    double *dmom = nullptr, *dcorr = nullptr;
    hmcg::KernelParams base{};
    // per-chunk timing events, two per chunk: around the sweep kernel(s) alone -- the copy-out of the last chunk rides the
    // same stream behind its kernel and is not kernel time.  (Created only when timing is requested; released on every path.)
    Events tev;

    size_t row(int i) const { return idx ? (size_t)idx[i] : (size_t)i; }
    // HMCG_TRACE=1 (diagnostics): host-side timeline of the call on stderr -- where the wall time beyond the kernels goes
    static bool trace_on() { static const bool on = diag_env("HMCG_TRACE") != nullptr; return on; }
    double ms_so_far() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count(); }
    void mark(const char* what) { if (trace_on()) trace.emplace_back(what, ms_so_far()); }

    int plan()
    {
        // HMCG_FAIL_DEVICE=id (diagnostics): the host entry fails on that device id before it touches anything -- lets a test
        // see hmcg_estimate_batch_multi report one worker's error while the others complete
        if (const char* fe = diag_env("HMCG_FAIL_DEVICE")) {
            if (atoi(fe) == c.device) { set_err("injected failure (HMCG_FAIL_DEVICE=%d)", c.device); return HMCG_E_NOMEM; }
        }
        int minT = 0;                                                  // the shortest valid window of this device's share
        for (int i = 0; h.T && i < n; ++i) {
            const int t = h.T[row(i)];
            if (t >= 2 && (minT == 0 || t < minT)) minT = t;
        }
        const HostLengths hl{h.T, idx, n};
        int rc = plan_call(cfg, h.ex, n, c.cu_count, minT, h.T ? &hl : nullptr, &pl);
        if (rc) return rc;
        if (!h.Y || !h.T) { set_err("Y and T are required"); return HMCG_E_BADARG; }
        const hmcg_extras* ex = h.ex;
        const size_t K = (size_t)cfg->K, ld = (size_t)cfg->ldY, H = (size_t)cfg->H, N = (size_t)n;
        const SweepSchedule& sch = pl.sched;
        nd_total = sch.nd;
        // (the sixth group, extras.pi_smooth_draws, is K * ldY columns wide: samples.pib[Nrun, N, D] of every window)
        const Col all[6] = { {h.mu, K, 0}, {h.sig2, K, 0}, {h.A, K * K, 0}, {h.pi_end, K, 0}, {h.fcast, 2 * H, 0},
                             {ex ? ex->pi_smooth_draws : nullptr, K * ld, 0} };
        want_corr = ex && ex->corr;                 // needs every draw column on the device, wanted by the caller or not
        for (int g = 0; g < 6; ++g) {
            Col& cc = cols[g] = all[g];
            if (!(cc.host || (want_corr && g != 5)) || nd_total == 0) cc.ncol = 0;
            if (cc.host && cc.ncol) copy_out = true;
            cc.off = ncols; ncols += cc.ncol;
        }
        stream_draws = ncols > 0;

        // chunk capacity: the ring of RING chunk buffers stays within ~1 GiB of device memory (and as much pinned memory)
        long long cap = nd_total > 0 ? nd_total : 1;
        if (stream_draws) {
            const long long budget = (1LL << 30) / RING / (long long)(8 * ncols * N);
            cap = std::max(1LL, std::min(cap, budget));
        }
        if (const char* cenv = diag_env("HMCG_CHUNK_DRAWS")) { const long long v = atoll(cenv); if (v > 0) cap = std::min(cap, v); }
        const bool one_chunk_env = diag_env("HMCG_NO_CHUNKS") != nullptr;           // diagnostics: one launch, as the device entry
        chunks = plan_chunks(sch.sweep_begin, sch.sweep_end, sch.per_sample, cfg->burnin, cfg->nrun, one_chunk_env ? (1LL << 40) : cap, stream_draws && !one_chunk_env,
                             diag_env("HMCG_CHUNK_FLOOR_DIV"), diag_env("HMCG_CHUNK_KEEP"));
        return 0;
    }

    // The table's rows first (the input block, the zeroed block, the other per-window arrays -- host_buffers), then the chunk
    // ring and the scratch of this plan.  (Every separate copy or memset is a node on the stream ahead of the first kernel:
    // ten of them cost more than the 2 MB of Y.)
    int lay_out()
    {
        const hmcg_extras* ex = h.ex;
        const bool need_ckpt = chunks.size() > 1 || (cfg->flags & HMCG_FLAG_RESUME) || (ex && (ex->xstate || ex->sumacc)) || !pl.sched.final_launch;
        bt = host_buffers(*cfg, h, n, need_ckpt, pl.needs_pif(), hmcg_host::moments_stride(cfg->K));
        long long chunk_max = 0;
        for (const Chunk& ch : chunks) chunk_max = std::max(chunk_max, ch.d1 - ch.d0);
        const size_t chunk_bytes = 8 * ncols * (size_t)n * (size_t)chunk_max;
        const int nring = stream_draws ? (int)std::min<size_t>(RING, chunks.size()) : 0;
        for (int r = 0; r < nring; ++r) o_dchunk[r] = bt.dev.add(chunk_bytes);
        const size_t o_dord = pl.nb > 1 ? bt.dev.add(bucket_list_bytes(n)) : 0;
        const size_t o_dfs = pl.bv ? bt.dev.add(scratch_bytes(pl, n, cfg->K)) : 0;
        const size_t o_dstr = pl.stream ? bt.dev.add(stream_bytes(pl, n)) : 0;
        o_pst0 = bt.pin.add(4 * (size_t)n);      // status words as they stand after the first launch: which windows were skipped
        for (int r = 0; r < nring; ++r) o_pchunk[r] = bt.pin.add(chunk_bytes);
        if (c.dev.ensure(bt.dev.total) || c.pin.ensure(bt.pin.total)) {
            set_err("workspace allocation failed (%zu B device, %zu B pinned)", bt.dev.total, bt.pin.total);
            return HMCG_E_NOMEM;
        }
        D = c.dev.base;
        P = c.pin.base;
        DevSlots ds = device_slots(bt, D);
        if (ds.ex.sigvals) ds.ex.nsave_ld = ex->nsave_ld;
        base = base_params(cfg, n, ds.Y, ds.T, ds.yreal, ds.status, &ds.ex, pl);
        base.summary = ds.summary;
        if (pl.bv) base.fscr = reinterpret_cast<double*>(D + o_dfs);
        if (pl.stream) { base.sscr = reinterpret_cast<uint8_t*>(D + o_dstr); base.stream_stride = (int64_t)slab_bytes(pl); }
        if (pl.nb > 1) dord = reinterpret_cast<int32_t*>(D + o_dord);
        dmom = ds.mom;
        dcorr = ds.ex.corr;
        return 0;
    }

    // Pack the rows idx[i] of the caller's arrays into pinned staging, send the input block (the first half of Y sets out
    // while the second half is packed: 2 MB at the headline shape), then either the RESUME state or one memset.
    int stage_inputs()
    {
        hipStream_t s = c.stream;
        const size_t N = (size_t)n, ybytes = bt.row[B_Y].bytes;       // Y at offset 0 of both arenas
        const int n_early = ybytes * N >= ((size_t)1 << 20) ? n / 2 : 0;
        const size_t sent = ybytes * n_early;
        pack_rows(bt, P, idx, 0, n_early);
        if (n_early > 0) { mark("half packed"); HIP_TRY(hipMemcpyAsync(D, P, sent, hipMemcpyHostToDevice, s)); mark("first half sent"); }
        pack_rows(bt, P, idx, n_early, n);
        mark("packed");
        HIP_TRY(hipMemcpyAsync(D + sent, P + sent, bt.input_bytes - sent, hipMemcpyHostToDevice, s));
        if (bt.resume) {
            // the chain state, then the running sums: sent from staging, or zeroed where the caller keeps none (sumacc)
            for (const bool ckpt : {true, false})
                for (const Buf& b : bt.row) {
                    if (!b.bytes || b.role != Role::inout || b.ckpt != ckpt) continue;
                    if (b.staged()) { HIP_TRY(hipMemcpyAsync(D + b.doff, P + b.poff, N * b.bytes, hipMemcpyHostToDevice, s)); }
                    else HIP_TRY(hipMemsetAsync(D + b.doff, 0, N * b.bytes, s));
                }
            // outputs a skipped window never writes read as zero
            for (const Buf& b : bt.row)
                if (b.bytes && b.zeroed && b.role == Role::out) HIP_TRY(hipMemsetAsync(D + b.doff, 0, N * b.bytes, s));
        } else {
            // status, summary, the checkpoint blocks (they live in the recycled arena: a skipped window writes none of them and
            // must not hand the caller an earlier call's bytes), x_final, sigvals, the per-sample summaries, pif, the running
            // smoothed / filtered sums: one memset
            HIP_TRY(hipMemsetAsync(D + bt.zero_begin, 0, bt.zero_end - bt.zero_begin, s));
        }
        if (pl.bv) HIP_TRY(hipFuncSetAttribute(pl.fptr(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.dyn));
        const int rc = dord ? build_bucket_lists(pl, base.T, n, dord, s) : 0;
        mark("inputs enqueued");
        return rc;
    }

    // Chunk cidx of pinned staging into the caller's per-draw arrays, shared with the scatter helpers.
    void scatter(int cidx)
    {
        const Chunk& ch = chunks[cidx];
        const size_t ndc = (size_t)(ch.d1 - ch.d0), N = (size_t)n, ld = (size_t)cfg->ldY;
        const double* src = reinterpret_cast<const double*>(P + o_pchunk[cidx % RING]);
        const int32_t* skip = reinterpret_cast<const int32_t*>(P + o_pst0);
        if (!copy_out || ndc == 0) return;
        const std::function<void(int, int)> part = [&](int pi, int np) {          // windows [i0, i1) of this chunk
            const int i0 = (int)((long long)n * pi / np), i1 = (int)((long long)n * (pi + 1) / np);
            for (int i = i0; i < i1; ++i) {
                const size_t g = row(i);
                // a skipped window produced nothing -- its block of the (recycled) chunk buffer holds an earlier call's bytes:
                // the contract (hmcg.h) says its outputs read zero
                const bool skipped = (skip[i] & bt.skip_mask) != 0;
                for (const Col& cc : cols) {
                    if (!cc.host) continue;
                    if (skipped) {
                        for (size_t q = 0; q < cc.ncol; ++q) memset(cc.host + (size_t)nd_total * (q + cc.ncol * g) + (size_t)ch.d0, 0, 8 * ndc);
                        continue;
                    }
                    const bool per_step = &cc == &cols[5];          // pi_smooth_draws: column = k * ldY + t; the kernel writes t < T[w] only
                    const size_t Tg = per_step ? (size_t)std::max(0, std::min((int)ld, (int)h.T[g])) : 0;
                    for (size_t q = 0; q < cc.ncol; ++q) {
                        double* dst = cc.host + (size_t)nd_total * (q + cc.ncol * g) + (size_t)ch.d0;
                        if (per_step && (q % ld) >= Tg) memset(dst, 0, 8 * ndc);              // beyond the window: reads zero
                        else memcpy(dst, src + ndc * (cc.off * N + q + cc.ncol * (size_t)i), 8 * ndc);
                    }
                }
            }
        };
        if (8 * ncols * N * ndc < ((size_t)1 << 20)) part(0, 1);                  // small chunks: not worth a hand-off
        else c.pool.run(part);
        mark("scattered");
    }

    // Kernel(s) of chunk cidx, then its copy-out: on the copy stream behind the kernel's event, or -- the last chunk, hidden
    // behind nothing -- on the compute stream itself right behind its kernel.  (An SDMA copy: 54 GB/s beside a running sweep
    // kernel.  Nothing small may go ahead of it on the copy stream: a copy of a few KB is a shader copy in the HIP runtime and
    // waits for a free CU, i.e. for the end of the NEXT sweep kernel.)
    int enqueue_chunk(int cidx)
    {
        hipStream_t s = c.stream;
        const int nch = (int)chunks.size();
        const Chunk& ch = chunks[cidx];
        const int slot = cidx % RING;
        hmcg::KernelParams p = base;
        p.sweep_begin = ch.s0; p.sweep_end = ch.s1;
        p.resume = (bt.resume || cidx > 0) ? 1 : 0;
        p.final_launch = (ch.s1 == pl.sched.total_sweeps) ? 1 : 0;
        const size_t ndc = (size_t)(ch.d1 - ch.d0), N = (size_t)n;
        p.nd_ld = (int32_t)std::max<size_t>(ndc, 1); p.draw_off = (int32_t)ch.d0;
        // The LAST chunk's draws (1/32 of the run, 1.3 MB at the headline shape) are written by the kernel straight into the
        // pinned staging buffer: host memory the device addresses directly, complete at the end of the kernel -- there is no
        // copy behind the last kernel (it cost ~0.1 ms of the call's tail: nothing left to hide it behind).  Only the last:
        // a kernel that writes across the link runs 11 % slower (measured with every chunk direct).
        const bool tail = cidx == nch - 1 && !want_corr;
        const bool direct_tail = stream_draws && copy_out && tail && nch > 1 && diag_env("HMCG_NO_DIRECT_TAIL") == nullptr;
        if (stream_draws) {
            double* cb = reinterpret_cast<double*>(direct_tail ? P + o_pchunk[slot] : D + o_dchunk[slot]);
            double** outs[6] = { &p.mu, &p.sig2, &p.A, &p.pi_end, &p.fcast, &p.pi_smooth_draws };
            for (int g = 0; g < 6; ++g) *outs[g] = cols[g].ncol ? cb + ndc * cols[g].off * N : nullptr;
            // (a skipped window writes nothing into its block: the scatter zeroes its rows of the caller's arrays instead of
            //  copying them -- no memset node per chunk on the stream)
        }
        // skips are decided in the first launch's prologue, which notes them in the host's skip words as well (pinned,
        // zeroed here): the scatter knows which windows' blocks hold nothing once that kernel has ended
        if (cidx == 0 && stream_draws && copy_out) {
            memset(P + o_pst0, 0, 4 * N);
            p.skip_host = reinterpret_cast<int32_t*>(P + o_pst0);
        }
        if (timing) HIP_TRY(hipEventRecord(tev.ev[2 * (size_t)cidx], s));
        const int rc = launch_kernel(c, pl, p, s, dord);
        if (rc) return rc;
        if (timing) HIP_TRY(hipEventRecord(tev.ev[2 * (size_t)cidx + 1], s));
        if (!stream_draws) return 0;
        hipStream_t cs = tail ? s : c.copy;
        if (!tail) {
            HIP_TRY(hipEventRecord(c.evk[slot], s));
            HIP_TRY(hipStreamWaitEvent(c.copy, c.evk[slot], 0));
        }
        if (ndc > 0 && copy_out && !direct_tail)
            HIP_TRY(hipMemcpyAsync(P + o_pchunk[slot], D + o_dchunk[slot], 8 * ncols * N * ndc, hipMemcpyDeviceToHost, cs));
        HIP_TRY(hipEventRecord(c.evc[slot], cs));
        if (want_corr && ndc > 0) {
            // second moments of the chunk's rounded draws, in HBM, beside the chunk's copy-out (calccorr)
            hmcg_host::MomentsArgs ma{p.mu, p.sig2, p.pi_end, p.A, p.fcast, dmom, (long long)ndc, (long long)ndc, n, cfg->K, cfg->H, ch.d0 == 0};
            HIP_TRY(hmcg_host::launch_moments(ma, s));
        }
        return 0;
    }

    // Behind the last kernel, on the compute stream: the correlations, then every returned row of the table (table order;
    // status | summary in one copy).
    int enqueue_returns()
    {
        mark("kernels enqueued");
        if (want_corr) HIP_TRY(hmcg_host::launch_corr_finalize(dmom, dcorr, n, cfg->K, c.stream));
        const size_t N = (size_t)n;
        size_t doff = 0, poff = 0, len = 0;
        for (const Buf& b : bt.row) {
            if (!b.returned()) continue;
            if (b.same_copy && len) { len = b.doff + N * b.bytes - doff; continue; }
            if (len) HIP_TRY(hipMemcpyAsync(P + poff, D + doff, len, hipMemcpyDeviceToHost, c.stream));
            doff = b.doff; poff = b.poff; len = N * b.bytes;
        }
        if (len) HIP_TRY(hipMemcpyAsync(P + poff, D + doff, len, hipMemcpyDeviceToHost, c.stream));
        return 0;
    }

    // The chunk pipeline: kernel c -> evk[c % RING] -> SDMA copy of its chunk buffer into pinned staging (copy stream) ->
    // evc[c % RING] -> host scatter into the caller's arrays.  A chunk buffer is [array][window][column][draw] with the chunk's
    // own draw count as leading dimension (one contiguous block: a plain 1-D copy, which the SDMA engines carry without touching
    // the CUs -- a helped sweep kernel leaves no registers for a blit kernel to run beside it).  Kernel c + RING reuses both
    // the device and the pinned buffer of chunk c: it is enqueued only after the host has waited for copy c and scattered it.
    int run_chunks()
    {
        const int nch = (int)chunks.size();
        if (timing) {
            tev.ev.assign(2 * (size_t)nch, nullptr);
            for (auto& e : tev.ev) HIP_TRY(hipEventCreate(&e));
        }
        int rc = 0;
        for (int enq = 0, sca = 0; enq < nch || (stream_draws && sca < nch);) {
            while (enq < nch && (!stream_draws || enq < sca + RING)) {
                if ((rc = enqueue_chunk(enq))) return rc;
                if (++enq == nch && (rc = enqueue_returns())) return rc;
            }
            if (!stream_draws) break;
            HIP_TRY(hipEventSynchronize(c.evc[sca % RING]));
            mark("copy landed");
            scatter(sca++);
        }
        mark("chunks scattered");
        return 0;
    }

    int collect_outputs()
    {
        HIP_TRY(hipStreamSynchronize(c.stream));
        mark("stream idle");
        unpack_rows(bt, P, idx, n);
        mark("small outputs copied");
        const int nch = (int)chunks.size();
        if (trace_on()) {
            fprintf(stderr, "[trace] device %d, %d windows, %d chunks:", c.device, n, nch);
            for (const auto& t : trace) fprintf(stderr, " %s %.3f |", t.first, t.second);
            if (timing) {
                fprintf(stderr, " chunk kernels (ms @ start after the first one's start):");
                for (int cidx = 0; cidx < nch; ++cidx) {
                    float ms = 0.f, at = 0.f;
                    (void)hipEventElapsedTime(&ms, tev.ev[2 * (size_t)cidx], tev.ev[2 * (size_t)cidx + 1]);
                    (void)hipEventElapsedTime(&at, tev.ev[0], tev.ev[2 * (size_t)cidx]);
                    fprintf(stderr, " %.3f@%.3f", ms, at);
                }
            }
            fprintf(stderr, "\n");
        }
        if (timing) {
            double kernel_ms = 0.0;
            for (int cidx = 0; cidx < nch; ++cidx) {
                float ms = 0.f;
                HIP_TRY(hipEventElapsedTime(&ms, tev.ev[2 * (size_t)cidx], tev.ev[2 * (size_t)cidx + 1]));
                kernel_ms += ms;       // the chunk's sweep kernel(s); a wait for a ring slot falls before the first event
            }
            fill_timing(timing, pl, c, kernel_ms, nch, ms_so_far(), n);
        }
        return 0;
    }
};

int run_host_on_device(DeviceCtx& c, const hmcg_config* cfg, const int32_t* idx, int n, const HostArrays& h, hmcg_timing* timing)
{
    HostCall k{c, cfg, idx, n, h, timing};
    int rc = k.plan();
    if (!rc) rc = k.lay_out();
    if (!rc) rc = k.stage_inputs();
    if (!rc) rc = k.run_chunks();
    if (!rc) rc = k.collect_outputs();
    return rc;
}

// ---- statistics of the draws: what the nine pairs of entries below share --------------------------------------------------------

// What a statistic's hmcg_timing says of its kernels beside the times and the launch count.
struct StatShape { int windows, threads_per_window, lds_bytes; };

void fill_stat_timing(hmcg_timing* t, const DeviceCtx& c, const StatShape& sh, double kernel_ms, int launches, double call_ms)
{
    memset(t, 0, sizeof *t);
    t->kernel_ms = kernel_ms; t->launches = launches; t->call_ms = call_ms;
    t->device = c.device; t->windows = sh.windows; t->buckets = 1;
    t->threads_per_window = sh.threads_per_window; t->lds_bytes = sh.lds_bytes;
}

// The frame of a statistic's device entry.  Its sums live in a context-owned arena (as the moment tables do): what `body`
// enqueues on `stream` is ordered behind the arena's last use on any stream (ev_scr) and becomes that last use.  With `timing`
// the call waits for the launches and reports their time.  Caller holds c.mu and has made c.device current.
template <class Body>
int stat_device(DeviceCtx& c, Arena& work, size_t work_bytes, hipStream_t stream, hmcg_timing* timing, const StatShape& sh, int launches,
                Body body)
{
    int rc = grow_shared(c, work, work_bytes);
    if (rc) return rc;
    HIP_TRY(hipStreamWaitEvent(stream, c.ev_scr, 0));
    if (timing) HIP_TRY(hipEventRecord(c.ev0, stream));
    if ((rc = body())) {
        (void)hipEventRecord(c.ev_scr, stream);          // what body did enqueue before it failed may be using the arena
        return rc;
    }
    HIP_TRY(hipEventRecord(c.ev_scr, stream));
    if (timing) {
        HIP_TRY(hipEventRecord(c.ev1, stream));
        HIP_TRY(hipEventSynchronize(c.ev1));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c.ev0, c.ev1));
        fill_stat_timing(timing, c, sh, ms, launches, 0.0);
    }
    return 0;
}

// Columns 0..cols-1 of src (leading dimension ld), draws [d0, d0 + n) of each, packed with leading dimension n; returns the end.
double* pack_columns(const double* src, size_t cols, size_t ld, long long d0, size_t n, double* dst)
{
    for (size_t q = 0; q < cols; ++q) memcpy(dst + q * n, src + q * ld + (size_t)d0, sizeof(double) * n);
    return dst + cols * n;
}

// The predictive mixture's draws [ch.d0, ch.d0 + ch.n) packed as its four features upload them: mu | sig2 | pi_end | A, each
// [W][columns][ch.n] (WK = W * K); returns the end.  Fan's range pass goes without the last two.
double* pack_mixture(const double* mu, const double* sig2, const double* pi_end, const double* A, size_t WK, size_t K, size_t ld,
                     const PredChunk& ch, bool with_pi, bool with_A, double* dst)
{
    dst = pack_columns(mu, WK, ld, ch.d0, (size_t)ch.n, dst);
    dst = pack_columns(sig2, WK, ld, ch.d0, (size_t)ch.n, dst);
    if (with_pi) dst = pack_columns(pi_end, WK, ld, ch.d0, (size_t)ch.n, dst);
    if (with_A) dst = pack_columns(A, WK * K, ld, ch.d0, (size_t)ch.n, dst);
    return dst;
}

// ... and a launch's arguments (PredictiveArgs, MixArgs, FanArgs) pointed at that chunk on the device.
template <class Args>
void place_mixture(Args& a, const PredChunk& ch, double* db, size_t WK, bool with_A)
{
    const size_t o_col = WK * (size_t)ch.n;
    a.mu = db; a.sig2 = db + o_col; a.pi_end = db + 2 * o_col; a.A = with_A ? db + 3 * o_col : nullptr;
    a.nd = ch.n; a.nd_ld = ch.n; a.slab0 = ch.d0 / PRED_SLAB;
}

// The upload ring of a statistic's host entry.  The draws go up in chunks of whole slabs (stat_plan.hpp; the scores: the
// windows in groups, a cut the entry makes itself): packed column by
// column into pinned staging (leading dimension = the chunk's draws), copied on the copy stream, reduced on the compute stream,
// RING buffers deep, so chunk c + 1 is packed and copied while chunk c's kernel runs.  Every chunk adds to the same sums in the
// work area; the caller finalizes at the end.  Both arenas are laid out once, before any pointer is taken: `io` (results and
// fixed inputs, at the same offsets in both) | work (device only) | the chunk buffers.
// Caller holds c.mu and has made c.device current.
struct UploadRing {
    DeviceCtx& c;
    hmcg_timing* timing;
    const std::chrono::steady_clock::time_point t_call = std::chrono::steady_clock::now();
    long long cdraws = 0;                            // draws of a full chunk (the ring's own cut)
    std::vector<PredChunk> chunks;
    int nbuf = 0;                                    // after alloc(): buffer pairs in use
    char *dev = nullptr, *pin = nullptr, *work = nullptr;    // after alloc(): the arenas and the device's work area
    double *dbuf[RING] = {}, *pbuf[RING] = {};
    size_t uploads = 0;                              // chunks uploaded so far, over every run(): the ring position
    Events tev;                                      // two per timed launch (only when timing is asked for)

    UploadRing(DeviceCtx& ctx, long long nd, int W, int ncol, hmcg_timing* t) : c(ctx), timing(t)
    {
        long long cap = 0;
        if (const char* cenv = diag_env("HMCG_CHUNK_DRAWS")) cap = atoll(cenv);
        cdraws = pred_chunk_draws(nd, W, ncol, cap);
        chunks = pred_chunks(nd, cdraws);
    }
    // ... or over a cut the caller has made: `ready` goes up chunk by chunk, whatever a chunk's {d0, n} counts.
    UploadRing(DeviceCtx& ctx, std::vector<PredChunk> ready, hmcg_timing* t) : c(ctx), timing(t), chunks(std::move(ready)) {}

    int alloc(const Layout& io, size_t work_bytes, size_t chunk_doubles)
    {
        nbuf = (int)std::min<size_t>(RING, chunks.size());
        Layout d = io, p = io;
        const size_t o_work = d.add(work_bytes);
        size_t o_d[RING] = {}, o_p[RING] = {};
        for (int b = 0; b < nbuf; ++b) { o_d[b] = d.add(sizeof(double) * chunk_doubles); o_p[b] = p.add(sizeof(double) * chunk_doubles); }
        if (c.dev.ensure(d.total) || c.pin.ensure(p.total)) {
            set_err("workspace allocation failed (%zu B device, %zu B pinned)", d.total, p.total);
            return HMCG_E_NOMEM;
        }
        dev = c.dev.base; pin = c.pin.base; work = dev + o_work;
        for (int b = 0; b < nbuf; ++b) { dbuf[b] = reinterpret_cast<double*>(dev + o_d[b]); pbuf[b] = reinterpret_cast<double*>(pin + o_p[b]); }
        return 0;
    }

    // enqueue() on the compute stream, between two events when the call is timed (a chunk's pair is created behind the enqueue
    // of its copy, so the copy hides it)
    template <class Enqueue>
    int timed(Enqueue enqueue)
    {
        if (!timing) return enqueue();
        hipEvent_t e[2] = {};
        for (hipEvent_t& x : e) { HIP_TRY(hipEventCreate(&x)); tev.ev.push_back(x); }
        HIP_TRY(hipEventRecord(e[0], c.stream));
        const int rc = enqueue();
        if (rc) return rc;
        HIP_TRY(hipEventRecord(e[1], c.stream));
        return 0;
    }

    // One pass over the chunks that start below `stop`: pack(chunk, pinned) fills the staging buffer and returns the doubles to
    // copy; launch(chunk, device, stream) enqueues the chunk's kernel.  A later run goes on where this one stood in the ring.
    template <class Pack, class Launch>
    int run(Pack pack, Launch launch, long long stop = LLONG_MAX)
    {
        for (const PredChunk& ch : chunks) {
            if (ch.d0 >= stop) break;
            const int b = (int)(uploads % (size_t)nbuf);
            if (uploads >= (size_t)nbuf) HIP_TRY(hipEventSynchronize(c.evk[b]));      // the kernel that read this buffer pair is done
            ++uploads;
            const size_t n = pack(ch, pbuf[b]);
            HIP_TRY(hipMemcpyAsync(dbuf[b], pbuf[b], sizeof(double) * n, hipMemcpyHostToDevice, c.copy));
            HIP_TRY(hipEventRecord(c.evc[b], c.copy));
            HIP_TRY(hipStreamWaitEvent(c.stream, c.evc[b], 0));
            const int rc = timed([&] { return launch(ch, dbuf[b], c.stream); });
            if (rc) return rc;
            HIP_TRY(hipEventRecord(c.evk[b], c.stream));
        }
        return 0;
    }

    // The results, `bytes` at offset `off` of `io`, into pinned staging behind everything on the compute stream; waits for them.
    int fetch(size_t off, size_t bytes)
    {
        HIP_TRY(hipMemcpyAsync(pin + off, dev + off, bytes, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        return 0;
    }

    int report(const StatShape& sh, int launches)
    {
        if (!timing) return 0;
        double kernel_ms = 0.0;
        for (size_t i = 0; i + 1 < tev.ev.size(); i += 2) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, tev.ev[i], tev.ev[i + 1]));
            kernel_ms += ms;
        }
        const double call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
        fill_stat_timing(timing, c, sh, kernel_ms, launches, call_ms);
        return 0;
    }
};

// ---- predictive CDFs of the regime mixture (predictive.hip; argument rules: predictive_plan.hpp; slab / chunk cut: stat_plan.hpp) ----

hmcg_host::PredictiveArgs predictive_args(const hmcg_predictive* p)
{
    hmcg_host::PredictiveArgs a{};
    a.W = p->W; a.K = p->K; a.G = p->G; a.n_h = p->n_h;
    fill_horizons(p->n_h, p->horizons, a.horizons);
    a.round5 = (p->flags & HMCG_PRED_ROUND5) != 0;
    a.nslab_total = pred_slabs(p->nd);
    return a;
}

StatShape predictive_shape(const hmcg_predictive* p) { return {p->W, 0, (int32_t)mixture_lds_bytes(p->K, p->n_h, mixture_max_horizon(*p) > 0)}; }

int predictive_device(DeviceCtx& c, const hmcg_predictive* p, const double* dmu, const double* dsig2, const double* dpi_end,
                      const double* dA, const double* dgrid, double* dcdf, hipStream_t stream, hmcg_timing* timing)
{
    const size_t work = sizeof(double) * predictive_part_doubles(p->W, p->nd, p->n_h, p->G);
    return stat_device(c, c.pred, work, stream, timing, predictive_shape(p), 2, [&]() -> int {
        hmcg_host::PredictiveArgs a = predictive_args(p);
        a.mu = dmu; a.sig2 = dsig2; a.pi_end = dpi_end; a.A = dA; a.grid = dgrid;
        a.part = reinterpret_cast<double*>(c.pred.base);
        a.nd = p->nd; a.nd_ld = p->nd_ld; a.slab0 = 0;
        HIP_TRY(launch_predictive(a, stream));
        HIP_TRY(launch_predictive_finalize(a.part, dcdf, p->W, p->n_h, p->G, p->nd, stream));
        return 0;
    });
}

// Host entry on one device, through the upload ring: every chunk adds its slabs' sums to the same table; one finalize at the end.
int predictive_host(DeviceCtx& c, const hmcg_predictive* p, const double* mu, const double* sig2, const double* pi_end, const double* A,
                    const double* grid, double* cdf, hmcg_timing* timing)
{
    const bool with_A = mixture_max_horizon(*p) > 0;
    const size_t WK = (size_t)p->W * (size_t)p->K, ld = (size_t)p->nd_ld;
    const int ncol = mixture_columns(p->K, with_A);
    UploadRing ring(c, p->nd, p->W, ncol, timing);
    const size_t b_grid = sizeof(double) * (size_t)p->G, b_cdf = sizeof(double) * (size_t)p->W * (size_t)p->n_h * (size_t)p->G;
    Layout io;
    const size_t o_grid = io.add(b_grid), o_cdf = io.add(b_cdf);
    const size_t work = sizeof(double) * predictive_part_doubles(p->W, p->nd, p->n_h, p->G);
    int rc = ring.alloc(io, work, (size_t)p->W * (size_t)ncol * (size_t)ring.cdraws);
    if (rc) return rc;
    memcpy(ring.pin + o_grid, grid, b_grid);
    HIP_TRY(hipMemcpyAsync(ring.dev + o_grid, ring.pin + o_grid, b_grid, hipMemcpyHostToDevice, c.stream));
    hmcg_host::PredictiveArgs a = predictive_args(p);
    a.grid = reinterpret_cast<double*>(ring.dev + o_grid); a.part = reinterpret_cast<double*>(ring.work);
    double* const dcdf = reinterpret_cast<double*>(ring.dev + o_cdf);
    rc = ring.run(
        [&](const PredChunk& ch, double* pb) { return (size_t)(pack_mixture(mu, sig2, pi_end, A, WK, (size_t)p->K, ld, ch, true, with_A, pb) - pb); },
        [&](const PredChunk& ch, double* db, hipStream_t s) -> int {
            place_mixture(a, ch, db, WK, with_A);
            HIP_TRY(launch_predictive(a, s));
            return 0;
        });
    if (rc) return rc;
    HIP_TRY(launch_predictive_finalize(a.part, dcdf, p->W, p->n_h, p->G, p->nd, c.stream));
    if ((rc = ring.fetch(o_cdf, b_cdf))) return rc;
    memcpy(cdf, ring.pin + o_cdf, b_cdf);
    return ring.report(predictive_shape(p), (int)ring.uploads + 1);
}

// ---- uncertainty-bias moments of the draws (bias.hip; argument rules: bias_plan.hpp; slab / chunk cut: stat_plan.hpp) ------------

hmcg_host::BiasArgs bias_args(const hmcg_bias* p)
{
    hmcg_host::BiasArgs a{};
    a.W = p->W; a.K = p->K; a.horizon = p->horizon; a.round5 = (p->flags & HMCG_BIAS_ROUND5) != 0;
    a.nslab_total = pred_slabs(p->nd);
    return a;
}

int bias_device(DeviceCtx& c, const hmcg_bias* p, const double* dmu, const double* dpi_end, const double* dA, const double* dfcast,
                double* dout, hipStream_t stream, hmcg_timing* timing)
{
    const size_t work = sizeof(double) * bias_part_doubles(p->W, p->nd, p->K);
    return stat_device(c, c.bias, work, stream, timing, {p->W, 256, 0}, 2, [&]() -> int {
        hmcg_host::BiasArgs a = bias_args(p);
        a.mu = dmu; a.pi_end = dpi_end; a.A = dA;
        a.fc = dfcast ? dfcast + p->nd_ld : nullptr;             // column 1: forecast_error of the first horizon
        a.fc_wstride = 2LL * p->H * p->nd_ld;
        a.part = reinterpret_cast<double*>(c.bias.base);
        a.nd = p->nd; a.nd_ld = p->nd_ld; a.slab0 = 0;
        HIP_TRY(launch_bias(a, stream));
        HIP_TRY(launch_bias_finalize(a.part, dout, p->W, p->K, p->nd, dfcast != nullptr, stream));
        return 0;
    });
}

// Host entry on one device, through the upload ring: every chunk files its slabs' sums in the same table (the first one the
// pivots too); one finalize at the end.
int bias_host(DeviceCtx& c, const hmcg_bias* p, const double* mu, const double* pi_end, const double* A, const double* fcast, double* out,
              hmcg_timing* timing)
{
    const int K = p->K, W = p->W;
    const bool with_A = p->horizon > 0, with_fc = fcast != nullptr;
    const size_t WK = (size_t)W * (size_t)K, ld = (size_t)p->nd_ld;
    const int ncol = bias_columns(*p, with_fc);
    UploadRing ring(c, p->nd, W, ncol, timing);
    const size_t b_out = sizeof(double) * (size_t)W * (size_t)HMCG_BIAS_STRIDE(K);
    Layout io;
    const size_t o_out = io.add(b_out);
    int rc = ring.alloc(io, sizeof(double) * bias_part_doubles(W, p->nd, K), (size_t)W * (size_t)ncol * (size_t)ring.cdraws);
    if (rc) return rc;
    hmcg_host::BiasArgs a = bias_args(p);
    a.part = reinterpret_cast<double*>(ring.work);
    // packed chunk: mu | pi_end | A | forecast error, each [W][columns][ch.n]
    rc = ring.run(
        [&](const PredChunk& ch, double* pb) {
            double* e = pack_columns(mu, WK, ld, ch.d0, (size_t)ch.n, pb);
            e = pack_columns(pi_end, WK, ld, ch.d0, (size_t)ch.n, e);
            if (with_A) e = pack_columns(A, WK * (size_t)K, ld, ch.d0, (size_t)ch.n, e);
            // column 1 of every window's 2H: forecast_error of the first horizon
            if (with_fc) e = pack_columns(fcast + ld, (size_t)W, 2 * (size_t)p->H * ld, ch.d0, (size_t)ch.n, e);
            return (size_t)(e - pb);
        },
        [&](const PredChunk& ch, double* db, hipStream_t s) -> int {
            const size_t o_pi = WK * (size_t)ch.n, o_A = 2 * o_pi, o_fc = o_A + (with_A ? o_pi * (size_t)K : 0);
            a.mu = db; a.pi_end = db + o_pi; a.A = with_A ? db + o_A : nullptr;
            a.fc = with_fc ? db + o_fc : nullptr; a.fc_wstride = ch.n;
            a.nd = ch.n; a.nd_ld = ch.n; a.slab0 = ch.d0 / PRED_SLAB;
            HIP_TRY(launch_bias(a, s));
            return 0;
        });
    if (rc) return rc;
    HIP_TRY(launch_bias_finalize(a.part, reinterpret_cast<double*>(ring.dev + o_out), W, K, p->nd, with_fc, c.stream));
    if ((rc = ring.fetch(o_out, b_out))) return rc;
    memcpy(out, ring.pin + o_out, b_out);
    return ring.report({W, 256, 0}, (int)ring.uploads + 1);
}

// ---- predictive-mixture moments of the draws (mixmoments.hip; argument rules and the walk: mixmoments_plan.hpp; slab / chunk cut:
// stat_plan.hpp) -----------------------------------------------------------------------------------------------------------------

hmcg_host::MixArgs mix_args(const hmcg_mixmom* p)
{
    hmcg_host::MixArgs a{};
    a.W = p->W; a.K = p->K; a.n_h = p->n_h; a.walk = mix_walk(*p); a.round5 = (p->flags & HMCG_MIX_ROUND5) != 0;
    a.nslab_total = pred_slabs(p->nd);
    return a;
}

int mix_device(DeviceCtx& c, const hmcg_mixmom* p, const double* dmu, const double* dsig2, const double* dpi_end, const double* dA,
               double* dout, hipStream_t stream, hmcg_timing* timing)
{
    const size_t work = sizeof(double) * mix_part_doubles(p->W, p->nd, p->n_h);
    return stat_device(c, c.mix, work, stream, timing, {p->W, 256, 0}, 2, [&]() -> int {
        hmcg_host::MixArgs a = mix_args(p);
        a.mu = dmu; a.sig2 = dsig2; a.pi_end = dpi_end; a.A = dA;
        a.part = reinterpret_cast<double*>(c.mix.base);
        a.nd = p->nd; a.nd_ld = p->nd_ld; a.slab0 = 0;
        HIP_TRY(launch_mixmoments(a, stream));
        HIP_TRY(launch_mixmoments_finalize(a.part, dout, p->W, p->n_h, p->nd, stream));
        return 0;
    });
}

// Host entry on one device, through the upload ring: every chunk files its slabs' sums in the same table (the first one the
// pivots too); one finalize at the end.
int mix_host(DeviceCtx& c, const hmcg_mixmom* p, const double* mu, const double* sig2, const double* pi_end, const double* A, double* out,
             hmcg_timing* timing)
{
    const int K = p->K, W = p->W;
    const bool with_A = mixture_max_horizon(*p) > 0;
    const size_t WK = (size_t)W * (size_t)K, ld = (size_t)p->nd_ld;
    const int ncol = mixture_columns(K, with_A);
    UploadRing ring(c, p->nd, W, ncol, timing);
    const size_t b_out = sizeof(double) * (size_t)W * (size_t)p->n_h * (size_t)HMCG_MIX_STRIDE;
    Layout io;
    const size_t o_out = io.add(b_out);
    int rc = ring.alloc(io, sizeof(double) * mix_part_doubles(W, p->nd, p->n_h), (size_t)W * (size_t)ncol * (size_t)ring.cdraws);
    if (rc) return rc;
    hmcg_host::MixArgs a = mix_args(p);
    a.part = reinterpret_cast<double*>(ring.work);
    rc = ring.run(
        [&](const PredChunk& ch, double* pb) { return (size_t)(pack_mixture(mu, sig2, pi_end, A, WK, (size_t)K, ld, ch, true, with_A, pb) - pb); },
        [&](const PredChunk& ch, double* db, hipStream_t s) -> int {
            place_mixture(a, ch, db, WK, with_A);
            HIP_TRY(launch_mixmoments(a, s));
            return 0;
        });
    if (rc) return rc;
    HIP_TRY(launch_mixmoments_finalize(a.part, reinterpret_cast<double*>(ring.dev + o_out), W, p->n_h, p->nd, c.stream));
    if ((rc = ring.fetch(o_out, b_out))) return rc;
    memcpy(out, ring.pin + o_out, b_out);
    return ring.report({W, 256, 0}, (int)ring.uploads + 1);
}

// ---- chain densities and running means of the draws (density.hip; argument rules, pieces and column groups: density_plan.hpp;
// chunk cut: stat_plan.hpp) -------------------------------------------------------------------------------------------------------

hmcg_host::DensArgs dens_args(const hmcg_density* p)
{
    hmcg_host::DensArgs a{};
    a.W = p->W; a.C = p->C; a.B = p->B; a.n_cuts = p->n_cuts; a.trace_len = p->trace_len; a.trace_stride = p->trace_stride;
    for (int j = 0; j < HMCG_MAXH; ++j) a.cuts[j] = j < p->n_cuts ? p->cuts[j] : 0;
    a.nd = p->nd; a.round5 = (p->flags & HMCG_DENS_ROUND5) != 0;
    return a;
}

int dens_device(DeviceCtx& c, const hmcg_density* p, const double* dx, const double* dlo_hi, double* drange, int64_t* dcounts,
                double* dstats, double* dtrace, hipStream_t stream, hmcg_timing* timing)
{
    const size_t work = dens_work_bytes(p->W, p->C, p->nd, p->cuts, p->n_cuts);
    return stat_device(c, c.dens, work, stream, timing, {p->W, 256, 0}, dlo_hi ? 3 : 4, [&]() -> int {
        hmcg_host::DensArgs a = dens_args(p);
        a.x = dx; a.work = c.dens.base; a.range = drange; a.counts = reinterpret_cast<unsigned long long*>(dcounts);
        a.stats = dstats; a.trace = dtrace; a.d_origin = 0; a.n = p->nd; a.nd_ld = p->nd_ld;
        HIP_TRY(launch_density_clear(a, stream));
        if (!dlo_hi) HIP_TRY(launch_density_range(a, stream));
        HIP_TRY(launch_density_resolve(a, dlo_hi, stream));
        HIP_TRY(launch_density_accumulate(a, stream));
        HIP_TRY(launch_density_finalize(a, stream));
        return 0;
    });
}

// Host entry on one device, through the upload ring.  Without lo_hi the bins need the range of ALL draws first: one pass of
// uploads for the range kernel, a second one for the counts and sums (chunks that lie wholly beyond the last cut and the running
// mean are not uploaded again); with lo_hi the second pass alone.  Both passes go through the one ring.
int dens_host(DeviceCtx& c, const hmcg_density* p, const double* x, const double* lo_hi, double* range, int64_t* counts, double* stats,
              double* trace, hmcg_timing* timing)
{
    const int W = p->W, C = p->C;
    const size_t wc = (size_t)W * (size_t)C, ld = (size_t)p->nd_ld;
    UploadRing ring(c, p->nd, W, C, timing);
    const size_t b_range = 8 * wc * 2, b_counts = 8 * wc * (size_t)p->n_cuts * (size_t)(p->B + DENS_SLOTS), b_stats = 8 * wc * (size_t)p->n_cuts * 2,
                 b_trace = 8 * wc * (size_t)p->trace_len;
    Layout io;
    const size_t o_range = io.add(b_range), o_counts = io.add(b_counts), o_stats = io.add(b_stats), o_trace = io.add(b_trace);
    const size_t b_out = io.total;               // the four results come back in one copy
    const size_t o_lohi = io.add(b_range);
    int rc = ring.alloc(io, dens_work_bytes(W, C, p->nd, p->cuts, p->n_cuts), wc * (size_t)ring.cdraws);
    if (rc) return rc;
    hmcg_host::DensArgs a = dens_args(p);
    a.work = ring.work;
    a.range = reinterpret_cast<double*>(ring.dev + o_range);
    a.counts = reinterpret_cast<unsigned long long*>(ring.dev + o_counts);
    a.stats = reinterpret_cast<double*>(ring.dev + o_stats);
    a.trace = reinterpret_cast<double*>(ring.dev + o_trace);
    // draws a second-pass chunk must reach below to matter: the last cut and the end of the running mean
    const long long reach = std::max<long long>(p->cuts[p->n_cuts - 1], (long long)p->trace_len * p->trace_stride);

    // the calls below must be enqueued on c.stream behind each other: clear, [range per chunk], resolve, accumulate per chunk, finalize
    a.x = ring.dbuf[0]; a.d_origin = 0; a.n = ring.chunks[0].n; a.nd_ld = ring.chunks[0].n;
    HIP_TRY(launch_density_clear(a, c.stream));
    for (int pass = lo_hi ? 1 : 0; pass < 2; ++pass) {
        if (pass == 1) {
            double* const dlohi = reinterpret_cast<double*>(ring.dev + o_lohi);
            if (lo_hi) {
                memcpy(ring.pin + o_lohi, lo_hi, b_range);
                HIP_TRY(hipMemcpyAsync(dlohi, ring.pin + o_lohi, b_range, hipMemcpyHostToDevice, c.stream));
            }
            HIP_TRY(launch_density_resolve(a, lo_hi ? dlohi : nullptr, c.stream));
        }
        rc = ring.run(
            [&](const PredChunk& ch, double* pb) { return (size_t)(pack_columns(x, wc, ld, ch.d0, (size_t)ch.n, pb) - pb); },
            [&](const PredChunk& ch, double* db, hipStream_t s) -> int {
                a.x = db; a.d_origin = ch.d0; a.n = ch.n; a.nd_ld = ch.n;
                HIP_TRY(pass == 0 ? launch_density_range(a, s) : launch_density_accumulate(a, s));
                return 0;
            },
            pass == 1 ? reach : LLONG_MAX);
        if (rc) return rc;
    }
    HIP_TRY(launch_density_finalize(a, c.stream));
    if ((rc = ring.fetch(0, b_out))) return rc;
    memcpy(range, ring.pin + o_range, b_range);
    memcpy(counts, ring.pin + o_counts, b_counts);
    memcpy(stats, ring.pin + o_stats, b_stats);
    if (b_trace) memcpy(trace, ring.pin + o_trace, b_trace);
    return ring.report({W, 256, 0}, (int)ring.uploads + 2);      // the chunks' kernels, resolve and finalize (the clear is not counted)
}

// ---- autocorrelation, effective sample size and split-R-hat of the draws (autocorr.hip; argument rules and thread split:
// autocorr_plan.hpp; chunk cut: stat_plan.hpp) ------------------------------------------------------------------------------------

hmcg_host::AcfArgs acf_args(const hmcg_autocorr* p)
{
    hmcg_host::AcfArgs a{};
    a.W = p->W; a.C = p->C; a.L = p->L; a.nd = p->nd; a.round5 = (p->flags & HMCG_ACF_ROUND5) != 0;
    return a;
}

int acf_device(DeviceCtx& c, const hmcg_autocorr* p, const double* dx, double* dacov, double* ddiag, hipStream_t stream, hmcg_timing* timing)
{
    return stat_device(c, c.acf, acf_work_bytes(p->W, p->C, p->L), stream, timing, {p->W, 256, 0}, 2, [&]() -> int {
        hmcg_host::AcfArgs a = acf_args(p);
        a.x = dx; a.work = c.acf.base; a.acov = dacov; a.diag = ddiag; a.d_origin = 0; a.n = p->nd; a.pre = 0; a.ld = p->nd_ld;
        HIP_TRY(launch_autocorr_accumulate(a, stream));
        HIP_TRY(launch_autocorr_finalize(a, stream));
        return 0;
    });
}

// Host entry on one device, through the upload ring in one pass.  Every chunk is packed with the min(L, d0) draws before it in
// front (the host holds the whole array), so the device carries nothing from chunk to chunk but the running sums, the pivot and
// the edge values in the work area.
int acf_host(DeviceCtx& c, const hmcg_autocorr* p, const double* x, double* acov, double* diag, hmcg_timing* timing)
{
    const int W = p->W, C = p->C, L = p->L;
    const size_t wc = (size_t)W * (size_t)C, ld = (size_t)p->nd_ld;
    UploadRing ring(c, p->nd, W, C, timing);
    const size_t b_acov = 8 * wc * (size_t)(L + 1), b_diag = 8 * wc * HMCG_ACF_STRIDE;
    Layout io;
    const size_t o_acov = io.add(b_acov), o_diag = io.add(b_diag);
    int rc = ring.alloc(io, acf_work_bytes(W, C, L), wc * (size_t)(ring.cdraws + L));
    if (rc) return rc;
    hmcg_host::AcfArgs a = acf_args(p);
    a.work = ring.work;
    a.acov = reinterpret_cast<double*>(ring.dev + o_acov);
    a.diag = reinterpret_cast<double*>(ring.dev + o_diag);
    rc = ring.run(
        [&](const PredChunk& ch, double* pb) {
            const long long pre = acf_pre(ch.d0, L);
            return (size_t)(pack_columns(x, wc, ld, ch.d0 - pre, (size_t)(pre + ch.n), pb) - pb);
        },
        [&](const PredChunk& ch, double* db, hipStream_t s) -> int {
            a.x = db; a.d_origin = ch.d0; a.n = ch.n; a.pre = acf_pre(ch.d0, L); a.ld = a.pre + ch.n;
            HIP_TRY(launch_autocorr_accumulate(a, s));
            return 0;
        });
    if (rc) return rc;
    // (the finalize kernel counts as kernel time here: it walks every lag of every column)
    if ((rc = ring.timed([&]() -> int { HIP_TRY(launch_autocorr_finalize(a, c.stream)); return 0; }))) return rc;
    if ((rc = ring.fetch(0, io.total))) return rc;
    memcpy(acov, ring.pin + o_acov, b_acov);
    memcpy(diag, ring.pin + o_diag, b_diag);
    return ring.report({W, 256, 0}, (int)ring.uploads + 1);
}

// ---- exact quantiles and credible limits of the draws (order.hip; argument rules, key, digit schedule and the cut of the columns
// into upload groups: order_plan.hpp; ABI: include/hmcg_order.h) ------------------------------------------------------------------

hmcg_host::OrdArgs ord_args(const hmcg_quantiles* p)
{
    hmcg_host::OrdArgs a{};
    a.nd = p->nd; a.Q = p->Q; a.round5 = (p->flags & HMCG_ORD_ROUND5) != 0;
    for (int i = 0; i < HMCG_ORD_MAXQ; ++i) a.probs[i] = i < p->Q ? p->probs[i] : 0.0;
    return a;
}

// The selection keeps everything in LDS: no work area, so nothing of the context is shared with an earlier call.
int ord_device(DeviceCtx& c, const hmcg_quantiles* p, const double* dx, double* dq, int64_t* dn, hipStream_t stream, hmcg_timing* timing)
{
    Arena none;
    return stat_device(c, none, 0, stream, timing, {p->W, 1024, ord_lds_bytes()}, 1, [&]() -> int {
        hmcg_host::OrdArgs a = ord_args(p);
        a.x = dx; a.q = dq; a.n = dn; a.ncols = (long long)p->W * p->C; a.ld = p->nd_ld;
        HIP_TRY(launch_chain_quantiles(a, stream));
        return 0;
    });
}

// Host entry on one device.  A selection needs its whole column resident, so this is not the draw-slab ring: the W * C columns
// go up in groups of whole columns (order_plan.hpp), packed with leading dimension nd into pinned staging, copied on the copy
// stream and selected on the compute stream, RING buffers deep: group g + 1 is packed and copied while group g's kernel runs.
// Every group writes its own rows of q and n, fetched once at the end.
int ord_host(DeviceCtx& c, const hmcg_quantiles* p, const double* x, double* q, int64_t* n, hmcg_timing* timing)
{
    const auto t_call = std::chrono::steady_clock::now();
    const long long wc = (long long)p->W * p->C;
    const size_t nd = (size_t)p->nd, ld = (size_t)p->nd_ld;
    long long cap = 0;
    if (const char* cenv = diag_env("HMCG_CHUNK_COLS")) cap = atoll(cenv);
    const std::vector<OrdGroup> groups = ord_groups(wc, ord_group_cols(p->nd, wc, cap));
    const int nbuf = (int)std::min<size_t>(RING, groups.size());
    const size_t b_q = sizeof(double) * (size_t)wc * (size_t)p->Q * HMCG_ORD_STRIDE, b_n = sizeof(int64_t) * (size_t)wc * 2;
    Layout d, h;
    const size_t o_q = d.add(b_q), o_n = d.add(b_n);
    h.add(b_q); h.add(b_n);
    size_t o_d[RING] = {}, o_p[RING] = {};
    const size_t b_group = sizeof(double) * (size_t)groups[0].n * nd;
    for (int b = 0; b < nbuf; ++b) { o_d[b] = d.add(b_group); o_p[b] = h.add(b_group); }
    if (c.dev.ensure(d.total) || c.pin.ensure(h.total)) {
        set_err("workspace allocation failed (%zu B device, %zu B pinned)", d.total, h.total);
        return HMCG_E_NOMEM;
    }
    Events tev;
    hmcg_host::OrdArgs a = ord_args(p);
    a.ld = p->nd;
    size_t up = 0;
    for (const OrdGroup& g : groups) {
        const int b = (int)(up % (size_t)nbuf);
        if (up >= (size_t)nbuf) HIP_TRY(hipEventSynchronize(c.evk[b]));          // the kernel that read this buffer pair is done
        ++up;
        double* pb = reinterpret_cast<double*>(c.pin.base + o_p[b]);
        double* db = reinterpret_cast<double*>(c.dev.base + o_d[b]);
        pack_columns(x + (size_t)g.c0 * ld, (size_t)g.n, ld, 0, nd, pb);
        HIP_TRY(hipMemcpyAsync(db, pb, sizeof(double) * (size_t)g.n * nd, hipMemcpyHostToDevice, c.copy));
        HIP_TRY(hipEventRecord(c.evc[b], c.copy));
        HIP_TRY(hipStreamWaitEvent(c.stream, c.evc[b], 0));
        hipEvent_t e[2] = {};
        if (timing) {
            for (hipEvent_t& ev : e) { HIP_TRY(hipEventCreate(&ev)); tev.ev.push_back(ev); }
            HIP_TRY(hipEventRecord(e[0], c.stream));
        }
        a.x = db; a.ncols = g.n;
        a.q = reinterpret_cast<double*>(c.dev.base + o_q) + (size_t)g.c0 * (size_t)p->Q * HMCG_ORD_STRIDE;
        a.n = reinterpret_cast<int64_t*>(c.dev.base + o_n) + (size_t)g.c0 * 2;
        HIP_TRY(launch_chain_quantiles(a, c.stream));
        if (timing) HIP_TRY(hipEventRecord(e[1], c.stream));
        HIP_TRY(hipEventRecord(c.evk[b], c.stream));
    }
    HIP_TRY(hipMemcpyAsync(c.pin.base + o_q, c.dev.base + o_q, o_n + b_n - o_q, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    memcpy(q, c.pin.base + o_q, b_q);
    memcpy(n, c.pin.base + o_n, b_n);
    if (timing) {
        double kernel_ms = 0.0;
        for (size_t i = 0; i + 1 < tev.ev.size(); i += 2) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, tev.ev[i], tev.ev[i + 1]));
            kernel_ms += ms;
        }
        const double call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
        fill_stat_timing(timing, c, {p->W, 1024, ord_lds_bytes()}, kernel_ms, (int)up, call_ms);
    }
    return 0;
}

// ---- ergodic regime law, durations and long-run moments of the draws (ergodic.hip; argument rules, work area and the per-draw
// arithmetic: ergodic_plan.hpp; slab / chunk cut: stat_plan.hpp; ABI: include/hmcg_ergodic.h) -------------------------------------

hmcg_host::ErgArgs erg_args(const hmcg_ergodic* p)
{
    hmcg_host::ErgArgs a{};
    a.W = p->W; a.K = p->K; a.round5 = (p->flags & HMCG_ERG_ROUND5) != 0;
    a.nslab_total = pred_slabs(p->nd);
    return a;
}

int erg_device(DeviceCtx& c, const hmcg_ergodic* p, const double* dmu, const double* dsig2, const double* dA, double* dcols, double* dout,
               int64_t* dn, hipStream_t stream, hmcg_timing* timing)
{
    const size_t work = sizeof(double) * erg_part_doubles(p->W, p->nd, p->K);
    return stat_device(c, c.erg, work, stream, timing, {p->W, 256, 0}, 2, [&]() -> int {
        hmcg_host::ErgArgs a = erg_args(p);
        a.mu = dmu; a.sig2 = dsig2; a.A = dA; a.cols = dcols;
        a.part = reinterpret_cast<double*>(c.erg.base);
        a.nd = p->nd; a.nd_ld = p->nd_ld; a.slab0 = 0;
        HIP_TRY(launch_ergodic(a, stream));
        HIP_TRY(launch_ergodic_finalize(a.part, dout, reinterpret_cast<long long*>(dn), p->W, p->K, p->nd, stream));
        return 0;
    });
}

// Host entry on one device, through the upload ring: every chunk files its slabs' sums in the same table (the first one the
// pivots too); one finalize at the end.  With cols a chunk buffer carries the chunk's per-draw columns behind its inputs: the
// kernel writes them there, they are copied to the pinned twin behind the kernel, and scattered into the caller's array when
// the ring comes back to that buffer (the ring has waited for the copy by then) or at the end.
int erg_host(DeviceCtx& c, const hmcg_ergodic* p, const double* mu, const double* sig2, const double* A, double* cols, double* out,
             int64_t* n, hmcg_timing* timing)
{
    const int K = p->K, W = p->W, C = erg_cols(K);
    const size_t WK = (size_t)W * (size_t)K, ld = (size_t)p->nd_ld;
    const int ncol = erg_columns(K) + (cols ? C : 0);
    UploadRing ring(c, p->nd, W, ncol, timing);
    const size_t b_out = sizeof(double) * (size_t)W * (size_t)C * 2, b_n = sizeof(int64_t) * (size_t)W * 2;
    Layout io;
    const size_t o_out = io.add(b_out), o_n = io.add(b_n);
    int rc = ring.alloc(io, sizeof(double) * erg_part_doubles(W, p->nd, K), (size_t)W * (size_t)ncol * (size_t)ring.cdraws);
    if (rc) return rc;
    hmcg_host::ErgArgs a = erg_args(p);
    a.part = reinterpret_cast<double*>(ring.work);
    const size_t in_cols = (size_t)W * (size_t)erg_columns(K);       // a chunk's columns ahead of its per-draw columns
    const PredChunk* held[RING] = {};                                // the chunk whose columns a buffer pair holds
    auto slot = [&] { return (int)((ring.uploads - 1) % (size_t)ring.nbuf); };      // the buffer pair of the chunk being packed / launched
    auto scatter = [&](int b) {
        if (!held[b]) return;
        const PredChunk& ch = *held[b];
        const double* src = ring.pbuf[b] + in_cols * (size_t)ch.n;
        for (size_t q = 0; q < (size_t)W * (size_t)C; ++q) memcpy(cols + q * ld + (size_t)ch.d0, src + q * (size_t)ch.n, sizeof(double) * (size_t)ch.n);
        held[b] = nullptr;
    };
    // packed chunk: mu | sig2 | A (its diagonal columns left as they are: never read), each [W][columns][ch.n], then cols [W][C][ch.n]
    rc = ring.run(
        [&](const PredChunk& ch, double* pb) {
            if (cols) scatter(slot());
            double* e = pack_columns(mu, WK, ld, ch.d0, (size_t)ch.n, pb);
            e = pack_columns(sig2, WK, ld, ch.d0, (size_t)ch.n, e);
            for (size_t q = 0; q < WK * (size_t)K; ++q) {
                const size_t ij = q % ((size_t)K * (size_t)K);
                if (ij % (size_t)K != ij / (size_t)K) memcpy(e + q * (size_t)ch.n, A + q * ld + (size_t)ch.d0, sizeof(double) * (size_t)ch.n);
            }
            e += WK * (size_t)K * (size_t)ch.n;
            return (size_t)(e - pb);
        },
        [&](const PredChunk& ch, double* db, hipStream_t s) -> int {
            const size_t o_col = WK * (size_t)ch.n;
            a.mu = db; a.sig2 = db + o_col; a.A = db + 2 * o_col; a.cols = cols ? db + in_cols * (size_t)ch.n : nullptr;
            a.nd = ch.n; a.nd_ld = ch.n; a.slab0 = ch.d0 / PRED_SLAB;
            HIP_TRY(launch_ergodic(a, s));
            if (cols) {
                const int b = slot();
                HIP_TRY(hipMemcpyAsync(ring.pbuf[b] + in_cols * (size_t)ch.n, a.cols, sizeof(double) * (size_t)W * (size_t)C * (size_t)ch.n,
                                       hipMemcpyDeviceToHost, s));
                held[b] = &ch;
            }
            return 0;
        });
    if (rc) return rc;
    HIP_TRY(launch_ergodic_finalize(a.part, reinterpret_cast<double*>(ring.dev + o_out), reinterpret_cast<long long*>(ring.dev + o_n), W, K,
                                    p->nd, c.stream));
    if ((rc = ring.fetch(0, io.total))) return rc;
    if (cols)
        for (int b = 0; b < ring.nbuf; ++b) scatter(b);
    memcpy(out, ring.pin + o_out, b_out);
    memcpy(n, ring.pin + o_n, b_n);
    return ring.report({W, 256, 0}, (int)ring.uploads + 1);
}

// ---- predictive quantiles of the regime mixture (fan.hip; argument rules, work area and the arithmetic outside the CDF:
// fan_plan.hpp; slab / chunk cut: stat_plan.hpp; ABI: include/hmcg_fan.h) -------------------------------------------------------------

hmcg_host::FanArgs fan_args(const hmcg_fan* p)
{
    hmcg_host::FanArgs a{};
    a.W = p->W; a.K = p->K; a.n_h = p->n_h; a.n_p = p->n_p;
    fill_horizons(p->n_h, p->horizons, a.horizons);
    for (int i = 0; i < HMCG_FAN_MAXP; ++i) a.probs[i] = i < p->n_p ? p->probs[i] : 0.0;
    a.round5 = (p->flags & HMCG_FAN_ROUND5) != 0;
    a.nslab_total = pred_slabs(p->nd);
    return a;
}

StatShape fan_shape(const hmcg_fan* p) { return {p->W, 0, (int32_t)mixture_lds_bytes(p->K, p->n_h, mixture_max_horizon(*p) > 0)}; }

int fan_device(DeviceCtx& c, const hmcg_fan* p, const double* dmu, const double* dsig2, const double* dpi_end, const double* dA, double* dout,
               double* drange, int32_t* dflag, hipStream_t stream, hmcg_timing* timing)
{
    const size_t work = sizeof(double) * fan_part_doubles(p->W, p->nd, p->n_h, p->n_p);
    const int R = fan_rounds(*p);
    return stat_device(c, c.fan, work, stream, timing, fan_shape(p), 2 + 2 * R, [&]() -> int {
        hmcg_host::FanArgs a = fan_args(p);
        a.mu = dmu; a.sig2 = dsig2; a.pi_end = dpi_end; a.A = dA; a.out = dout; a.range = drange; a.flag = dflag;
        a.part = reinterpret_cast<double*>(c.fan.base);
        a.nd = p->nd; a.nd_ld = p->nd_ld; a.slab0 = 0;
        HIP_TRY(launch_fan_range(a, stream));
        HIP_TRY(launch_fan_range_finalize(a, stream));
        for (int r = 1; r <= R; ++r) {
            HIP_TRY(launch_fan_eval(a, r, stream));
            HIP_TRY(launch_fan_step(a, r, r == R, p->nd, stream));
        }
        return 0;
    });
}

// Host entry on one device: R + 1 passes of the upload ring, which keeps its position from one pass to the next -- the range
// pass (mu and sig2 alone), then one pass per round, each followed on the compute stream by the kernel that closes it.  The
// brackets stay on the device between the passes; out, range and flag come back once, at the end.
int fan_host(DeviceCtx& c, const hmcg_fan* p, const double* mu, const double* sig2, const double* pi_end, const double* A, double* out,
             double* range, int32_t* flag, hmcg_timing* timing)
{
    const bool with_A = mixture_max_horizon(*p) > 0;
    const size_t WK = (size_t)p->W * (size_t)p->K, ld = (size_t)p->nd_ld;
    const int ncol = mixture_columns(p->K, with_A), R = fan_rounds(*p);
    UploadRing ring(c, p->nd, p->W, ncol, timing);
    const size_t n_q = (size_t)p->W * (size_t)p->n_h * (size_t)p->n_p;
    const size_t b_out = sizeof(double) * n_q * HMCG_FAN_STRIDE, b_range = sizeof(double) * (size_t)p->W * 2, b_flag = sizeof(int32_t) * n_q;
    Layout io;
    const size_t o_out = io.add(b_out), o_range = io.add(b_range), o_flag = io.add(b_flag);
    int rc = ring.alloc(io, sizeof(double) * fan_part_doubles(p->W, p->nd, p->n_h, p->n_p), (size_t)p->W * (size_t)ncol * (size_t)ring.cdraws);
    if (rc) return rc;
    hmcg_host::FanArgs a = fan_args(p);
    a.part = reinterpret_cast<double*>(ring.work);
    a.out = reinterpret_cast<double*>(ring.dev + o_out); a.range = reinterpret_cast<double*>(ring.dev + o_range);
    a.flag = reinterpret_cast<int32_t*>(ring.dev + o_flag);
    // the range pass uploads mu | sig2 alone
    rc = ring.run(
        [&](const PredChunk& ch, double* pb) { return (size_t)(pack_mixture(mu, sig2, pi_end, A, WK, (size_t)p->K, ld, ch, false, false, pb) - pb); },
        [&](const PredChunk& ch, double* db, hipStream_t s) -> int {
            place_mixture(a, ch, db, WK, with_A);
            HIP_TRY(launch_fan_range(a, s));
            return 0;
        });
    if (rc) return rc;
    HIP_TRY(launch_fan_range_finalize(a, c.stream));
    for (int r = 1; r <= R; ++r) {
        rc = ring.run(
            [&](const PredChunk& ch, double* pb) { return (size_t)(pack_mixture(mu, sig2, pi_end, A, WK, (size_t)p->K, ld, ch, true, with_A, pb) - pb); },
            [&](const PredChunk& ch, double* db, hipStream_t s) -> int {
                place_mixture(a, ch, db, WK, with_A);
                HIP_TRY(launch_fan_eval(a, r, s));
                return 0;
            });
        if (rc) return rc;
        HIP_TRY(launch_fan_step(a, r, r == R, p->nd, c.stream));
    }
    if ((rc = ring.fetch(0, io.total))) return rc;
    memcpy(out, ring.pin + o_out, b_out);
    memcpy(range, ring.pin + o_range, b_range);
    memcpy(flag, ring.pin + o_flag, b_flag);
    return ring.report(fan_shape(p), (int)ring.uploads + 1 + R);
}

// ---- proper scores of the predictive regime mixture (score.hip; thinning, tiles, work area, window groups, argument rules and
// the per-term arithmetic: score_plan.hpp; ABI: include/hmcg_score.h) -----------------------------------------------------------

hmcg_host::ScoreArgs score_args(const hmcg_score* p)
{
    hmcg_host::ScoreArgs a{};
    a.K = p->K; a.n_h = p->n_h; a.n_u = score_used(*p);
    fill_horizons(p->n_h, p->horizons, a.horizons);
    a.round5 = (p->flags & HMCG_SCORE_ROUND5) != 0;
    a.yreal_ld = p->W;
    return a;
}

StatShape score_shape(const hmcg_score* p) { return {p->W, SCORE_TP, (int32_t)score_lds_bytes(p->K, p->n_h, mixture_max_horizon(*p) > 0)}; }

int score_launches(const hmcg_host::ScoreArgs& a, hipStream_t stream)
{
    HIP_TRY(launch_score_components(a, stream));
    HIP_TRY(launch_score_pairs(a, stream));
    HIP_TRY(launch_score_finish(a, stream));
    return 0;
}

int score_device(DeviceCtx& c, const hmcg_score* p, const double* dmu, const double* dsig2, const double* dpi_end, const double* dA,
                 const double* dyreal, double* dout, hipStream_t stream, hmcg_timing* timing)
{
    const size_t work = sizeof(double) * score_work_doubles(p->W, score_used(*p), p->K, p->n_h);
    return stat_device(c, c.score, work, stream, timing, score_shape(p), 3, [&]() -> int {
        hmcg_host::ScoreArgs a = score_args(p);
        a.mu = dmu; a.sig2 = dsig2; a.pi_end = dpi_end; a.A = dA; a.yreal = dyreal; a.out = dout;
        a.work = reinterpret_cast<double*>(c.score.base);
        a.W = p->W; a.w0 = 0; a.stride = score_stride(p->nd, p->stride); a.nd_ld = p->nd_ld;
        return score_launches(a, stream);
    });
}

// Host entry on one device.  The pair pass needs a window's used draws resident, so the upload ring goes over window groups
// and not over draw slabs: only the draws u * stride are read, packed with leading dimension n_u into pinned staging (per
// group: mu | sig2 | pi_end | A, each [windows][columns][n_u]); group g + 1 is packed and copied while group g's kernels run.
// Windows are independent and every group writes its own rows of out, fetched once at the end.
int score_host(DeviceCtx& c, const hmcg_score* p, const double* mu, const double* sig2, const double* pi_end, const double* A,
               const double* yreal, double* out, hmcg_timing* timing)
{
    const bool with_A = mixture_max_horizon(*p) > 0;
    const long long n_u = score_used(*p), stride = score_stride(p->nd, p->stride);
    const size_t K = (size_t)p->K, ld = (size_t)p->nd_ld;
    const int ncol = mixture_columns(p->K, with_A);
    long long cap = 0;
    if (const char* cenv = diag_env("HMCG_SCORE_GROUP_WINDOWS")) cap = atoll(cenv);
    const int gw = score_group_windows(p->W, n_u, ncol, cap);
    UploadRing ring(c, pred_chunks(p->W, gw), timing);           // a chunk {d0, n}: windows [d0, d0 + n)
    const size_t b_y = sizeof(double) * (size_t)p->n_h * (size_t)p->W, b_out = sizeof(double) * (size_t)p->W * (size_t)p->n_h * HMCG_SCORE_STRIDE;
    Layout io;
    const size_t o_y = io.add(b_y), o_out = io.add(b_out);
    int rc = ring.alloc(io, sizeof(double) * score_work_doubles(gw, n_u, p->K, p->n_h), (size_t)gw * (size_t)ncol * (size_t)n_u);
    if (rc) return rc;
    memcpy(ring.pin + o_y, yreal, b_y);
    HIP_TRY(hipMemcpyAsync(ring.dev + o_y, ring.pin + o_y, b_y, hipMemcpyHostToDevice, c.stream));
    hmcg_host::ScoreArgs a = score_args(p);
    a.yreal = reinterpret_cast<const double*>(ring.dev + o_y);
    a.work = reinterpret_cast<double*>(ring.work);
    a.stride = 1; a.nd_ld = n_u;
    // every stride-th draw of `cols` columns of the group's windows
    auto pack = [&](const double* src, size_t cols, const PredChunk& g, double* dst) {
        for (size_t q = 0; q < (size_t)g.n * cols; ++q) {
            const double* col = src + ((size_t)g.d0 * cols + q) * ld;
            if (stride == 1) memcpy(dst, col, sizeof(double) * (size_t)n_u);
            else for (long long u = 0; u < n_u; ++u) dst[u] = col[(size_t)u * (size_t)stride];
            dst += n_u;
        }
        return dst;
    };
    rc = ring.run(
        [&](const PredChunk& g, double* pb) {
            double* e = pack(mu, K, g, pb);
            e = pack(sig2, K, g, e);
            e = pack(pi_end, K, g, e);
            if (with_A) e = pack(A, K * K, g, e);
            return (size_t)(e - pb);
        },
        [&](const PredChunk& g, double* db, hipStream_t s) -> int {
            const size_t o_col = (size_t)g.n * K * (size_t)n_u;
            a.mu = db; a.sig2 = db + o_col; a.pi_end = db + 2 * o_col; a.A = with_A ? db + 3 * o_col : nullptr;
            a.W = (int)g.n; a.w0 = g.d0;
            a.out = reinterpret_cast<double*>(ring.dev + o_out) + (size_t)g.d0 * (size_t)p->n_h * HMCG_SCORE_STRIDE;
            return score_launches(a, s);
        });
    if (rc) return rc;
    if ((rc = ring.fetch(o_out, b_out))) return rc;
    memcpy(out, ring.pin + o_out, b_out);
    return ring.report(score_shape(p), 3 * (int)ring.uploads);
}

// The prologue of a compute entry on one device.  The argument check comes first and needs no device: a caller on a machine
// without one still gets the argument errors.  Then the context of p->device, its lock, the device made current, and body(context).
template <class P, class Check, class Body>
int entry(const P* p, Check check, Body body)
{
    g_err[0] = 0;
    char msg[160];
    int rc = check(msg, sizeof msg);
    if (rc) { set_err("%s", msg); return rc; }
    DeviceCtx* c = nullptr;
    if ((rc = get_context(p->device, &c))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->phys));
    return body(*c);
}

}  // namespace

extern "C" {

int hmcg_version(void) { return HMCG_VERSION; }

int hmcg_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    if (n > 0 && virtual_devices() > 0) return virtual_devices();
    return n;
}

const char* hmcg_last_error(void) { return g_err; }

void hmcg_shutdown(void)
{
    std::lock_guard<std::mutex> lk(g_init_mu);
    for (DeviceCtx& c : g_ctx) {
        std::lock_guard<std::mutex> lc(c.mu);
        destroy_context(c);
    }
}

int hmcg_estimate_batch_device(const hmcg_config* cfg, const double* dY, const int32_t* dT, const double* dyreal,
                               double* dmu, double* dsig2, double* dA, double* dpi_end, double* dfcast,
                               double* dsummary, int32_t* dstatus, const hmcg_extras* dextras, void* stream,
                               hmcg_timing* timing)
{
    return entry(cfg, [&](char* msg, size_t n) { return validate(cfg, msg, n); }, [&](DeviceCtx& c) {
        hipStream_t s = stream ? (hipStream_t)stream : c.stream;
        return launch_device(c, cfg, dY, dT, dyreal, dmu, dsig2, dA, dpi_end, dfcast, dsummary, dstatus, dextras, s, timing);
    });
}

int hmcg_estimate_batch(const hmcg_config* cfg, const double* Y, const int32_t* T, const double* yreal, double* mu,
                        double* sig2, double* A, double* pi_end, double* fcast, double* summary, int32_t* status,
                        const hmcg_extras* extras, hmcg_timing* timing)
{
    return entry(cfg, [&](char* msg, size_t n) { return validate(cfg, msg, n); }, [&](DeviceCtx& c) {
        const HostArrays h{Y, T, yreal, mu, sig2, A, pi_end, fcast, summary, status, extras};
        return run_host_on_device(c, cfg, nullptr, cfg->W, h, timing);
    });
}

int hmcg_estimate_batch_multi(const hmcg_config* cfg, int32_t n_devices, const int32_t* device_ids, const double* Y,
                              const int32_t* T, const double* yreal, double* mu, double* sig2, double* A, double* pi_end,
                              double* fcast, double* summary, int32_t* status, const hmcg_extras* extras, hmcg_timing* timing)
{
    g_err[0] = 0;
    char msg[160];
    int rc = validate(cfg, msg, sizeof msg);
    if (rc) { set_err("%s", msg); return rc; }
    if (!Y || !T) { set_err("Y and T are required"); return HMCG_E_BADARG; }
    if (n_devices < 1 || n_devices > HMCG_MAXDEV) { set_err("n_devices %d out of range (1..%d)", n_devices, HMCG_MAXDEV); return HMCG_E_BADARG; }
    std::vector<int32_t> devs((size_t)n_devices);
    for (int i = 0; i < n_devices; ++i) devs[(size_t)i] = device_ids ? device_ids[i] : i;
    for (int i = 0; i < n_devices; ++i)
        for (int j = 0; j < i; ++j)
            if (devs[(size_t)i] == devs[(size_t)j]) { set_err("device %d listed twice", devs[(size_t)i]); return HMCG_E_BADARG; }
    const int G = std::min<int>(n_devices, cfg->W);                 // never more devices than windows
    const auto parts = partition_windows(T, cfg->W, G);
    const HostArrays h{Y, T, yreal, mu, sig2, A, pi_end, fcast, summary, status, extras};
    std::vector<int> rcs((size_t)G, 0);
    std::vector<std::string> errs((size_t)G);
    if (timing) memset(timing, 0, sizeof(hmcg_timing) * (size_t)n_devices);
    auto worker = [&](int r) {
        g_err[0] = 0;
        DeviceCtx* c = nullptr;
        int rr = get_context(devs[(size_t)r], &c);
        if (!rr) {
            std::lock_guard<std::mutex> lk(c->mu);
            hipError_t e = hipSetDevice(c->phys);
            if (e != hipSuccess) { set_err("hipSetDevice(%d) failed: %s", c->phys, hipGetErrorString(e)); rr = (int)e; }
            else rr = run_host_on_device(*c, cfg, parts[(size_t)r].data(), (int)parts[(size_t)r].size(), h, timing ? timing + r : nullptr);
        }
        rcs[(size_t)r] = rr;
        errs[(size_t)r] = g_err;           // thread-local message of this worker
    };
    if (G == 1) {
        worker(0);
    } else {
        std::vector<std::thread> th;
        th.reserve((size_t)G);
        for (int r = 0; r < G; ++r) th.emplace_back(worker, r);
        for (auto& t : th) t.join();
    }
    for (int r = 0; r < G; ++r)
        if (rcs[(size_t)r]) {
            set_err("device %d: %s", devs[(size_t)r], errs[(size_t)r].c_str());
            return rcs[(size_t)r];
        }
    return 0;
}

int hmcg_predictive_cdf_device(const hmcg_predictive* p, const double* dmu, const double* dsig2, const double* dpi_end, const double* dA,
                               const double* dgrid, double* dcdf, void* stream, hmcg_timing* timing)
{
    return entry(p, [&](char* msg, size_t n) { return check_predictive(p, dmu, dsig2, dpi_end, dA, dgrid, dcdf, false, msg, n); },
                 [&](DeviceCtx& c) {
        return predictive_device(c, p, dmu, dsig2, dpi_end, dA, dgrid, dcdf, stream ? (hipStream_t)stream : c.stream, timing);
    });
}

int hmcg_predictive_cdf(const hmcg_predictive* p, const double* mu, const double* sig2, const double* pi_end, const double* A,
                        const double* grid, double* cdf, hmcg_timing* timing)
{
    return entry(p, [&](char* msg, size_t n) { return check_predictive(p, mu, sig2, pi_end, A, grid, cdf, true, msg, n); },
                 [&](DeviceCtx& c) { return predictive_host(c, p, mu, sig2, pi_end, A, grid, cdf, timing); });
}

int hmcg_bias_moments_device(const hmcg_bias* p, const double* dmu, const double* dpi_end, const double* dA, const double* dfcast,
                             double* dout, void* stream, hmcg_timing* timing)
{
    return entry(p, [&](char* msg, size_t n) { return check_bias(p, dmu, dpi_end, dA, dfcast, dout, msg, n); }, [&](DeviceCtx& c) {
        return bias_device(c, p, dmu, dpi_end, dA, dfcast, dout, stream ? (hipStream_t)stream : c.stream, timing);
    });
}

int hmcg_bias_moments(const hmcg_bias* p, const double* mu, const double* pi_end, const double* A, const double* fcast, double* out,
                      hmcg_timing* timing)
{
    return entry(p, [&](char* msg, size_t n) { return check_bias(p, mu, pi_end, A, fcast, out, msg, n); },
                 [&](DeviceCtx& c) { return bias_host(c, p, mu, pi_end, A, fcast, out, timing); });
}

int hmcg_mixture_moments_device(const hmcg_mixmom* p, const double* dmu, const double* dsig2, const double* dpi_end, const double* dA,
                                double* dout, void* stream, hmcg_timing* timing)
{
    return entry(p, [&](char* msg, size_t n) { return check_mixmom(p, dmu, dsig2, dpi_end, dA, dout, msg, n); }, [&](DeviceCtx& c) {
        return mix_device(c, p, dmu, dsig2, dpi_end, dA, dout, stream ? (hipStream_t)stream : c.stream, timing);
    });
}

int hmcg_mixture_moments(const hmcg_mixmom* p, const double* mu, const double* sig2, const double* pi_end, const double* A, double* out,
                         hmcg_timing* timing)
{
    return entry(p, [&](char* msg, size_t n) { return check_mixmom(p, mu, sig2, pi_end, A, out, msg, n); },
                 [&](DeviceCtx& c) { return mix_host(c, p, mu, sig2, pi_end, A, out, timing); });
}

int hmcg_chain_density_device(const hmcg_density* p, const double* dx, const double* dlo_hi, double* drange, int64_t* dcounts,
                              double* dstats, double* dtrace, void* stream, hmcg_timing* timing)
{
    return entry(p, [&](char* msg, size_t n) { return check_density(p, dx, dlo_hi, drange, dcounts, dstats, dtrace, false, msg, n); },
                 [&](DeviceCtx& c) {
        return dens_device(c, p, dx, dlo_hi, drange, dcounts, dstats, dtrace, stream ? (hipStream_t)stream : c.stream, timing);
    });
}

int hmcg_chain_density(const hmcg_density* p, const double* x, const double* lo_hi, double* range, int64_t* counts, double* stats,
                       double* trace, hmcg_timing* timing)
{
    return entry(p, [&](char* msg, size_t n) { return check_density(p, x, lo_hi, range, counts, stats, trace, true, msg, n); },
                 [&](DeviceCtx& c) { return dens_host(c, p, x, lo_hi, range, counts, stats, trace, timing); });
}

int hmcg_chain_autocorr_device(const hmcg_autocorr* p, const double* dx, double* dacov, double* ddiag, void* stream, hmcg_timing* timing)
{
    return entry(p, [&](char* msg, size_t n) { return check_autocorr(p, dx, dacov, ddiag, msg, n); },
                 [&](DeviceCtx& c) { return acf_device(c, p, dx, dacov, ddiag, stream ? (hipStream_t)stream : c.stream, timing); });
}

int hmcg_chain_autocorr(const hmcg_autocorr* p, const double* x, double* acov, double* diag, hmcg_timing* timing)
{
    return entry(p, [&](char* msg, size_t n) { return check_autocorr(p, x, acov, diag, msg, n); },
                 [&](DeviceCtx& c) { return acf_host(c, p, x, acov, diag, timing); });
}

int hmcg_chain_quantiles_device(const hmcg_quantiles* p, const double* dx, double* dq, int64_t* dn, void* stream, hmcg_timing* timing)
{
    return entry(p, [&](char* msg, size_t n) { return check_quantiles(p, dx, dq, dn, msg, n); },
                 [&](DeviceCtx& c) { return ord_device(c, p, dx, dq, dn, stream ? (hipStream_t)stream : c.stream, timing); });
}

int hmcg_chain_quantiles(const hmcg_quantiles* p, const double* x, double* q, int64_t* n, hmcg_timing* timing)
{
    return entry(p, [&](char* msg, size_t nmsg) { return check_quantiles(p, x, q, n, msg, nmsg); },
                 [&](DeviceCtx& c) { return ord_host(c, p, x, q, n, timing); });
}

int hmcg_ergodic_moments_device(const hmcg_ergodic* p, const double* dmu, const double* dsig2, const double* dA, double* dcols, double* dout,
                                int64_t* dn, void* stream, hmcg_timing* timing)
{
    return entry(p, [&](char* msg, size_t nmsg) { return check_ergodic(p, dmu, dsig2, dA, dout, dn, msg, nmsg); }, [&](DeviceCtx& c) {
        return erg_device(c, p, dmu, dsig2, dA, dcols, dout, dn, stream ? (hipStream_t)stream : c.stream, timing);
    });
}

int hmcg_ergodic_moments(const hmcg_ergodic* p, const double* mu, const double* sig2, const double* A, double* cols, double* out, int64_t* n,
                         hmcg_timing* timing)
{
    return entry(p, [&](char* msg, size_t nmsg) { return check_ergodic(p, mu, sig2, A, out, n, msg, nmsg); },
                 [&](DeviceCtx& c) { return erg_host(c, p, mu, sig2, A, cols, out, n, timing); });
}

int hmcg_predictive_quantiles_device(const hmcg_fan* p, const double* dmu, const double* dsig2, const double* dpi_end, const double* dA,
                                     double* dout, double* drange, int32_t* dflag, void* stream, hmcg_timing* timing)
{
    return entry(p, [&](char* msg, size_t nmsg) { return check_fan(p, dmu, dsig2, dpi_end, dA, dout, drange, dflag, msg, nmsg); },
                 [&](DeviceCtx& c) {
        return fan_device(c, p, dmu, dsig2, dpi_end, dA, dout, drange, dflag, stream ? (hipStream_t)stream : c.stream, timing);
    });
}

int hmcg_predictive_quantiles(const hmcg_fan* p, const double* mu, const double* sig2, const double* pi_end, const double* A, double* out,
                              double* range, int32_t* flag, hmcg_timing* timing)
{
    return entry(p, [&](char* msg, size_t nmsg) { return check_fan(p, mu, sig2, pi_end, A, out, range, flag, msg, nmsg); },
                 [&](DeviceCtx& c) { return fan_host(c, p, mu, sig2, pi_end, A, out, range, flag, timing); });
}

int hmcg_predictive_scores_device(const hmcg_score* p, const double* dmu, const double* dsig2, const double* dpi_end, const double* dA,
                                  const double* dyreal, double* dout, void* stream, hmcg_timing* timing)
{
    return entry(p, [&](char* msg, size_t nmsg) { return check_score(p, dmu, dsig2, dpi_end, dA, dyreal, dout, msg, nmsg); }, [&](DeviceCtx& c) {
        return score_device(c, p, dmu, dsig2, dpi_end, dA, dyreal, dout, stream ? (hipStream_t)stream : c.stream, timing);
    });
}

int hmcg_predictive_scores(const hmcg_score* p, const double* mu, const double* sig2, const double* pi_end, const double* A,
                           const double* yreal, double* out, hmcg_timing* timing)
{
    return entry(p, [&](char* msg, size_t nmsg) { return check_score(p, mu, sig2, pi_end, A, yreal, out, msg, nmsg); },
                 [&](DeviceCtx& c) { return score_host(c, p, mu, sig2, pi_end, A, yreal, out, timing); });
}

}  // extern "C"
