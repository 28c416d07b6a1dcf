// stat_device.hpp -- the kernel pieces the draw statistics share (predictive.hip, bias.hip, mixmoments.hip, density.hip,
// autocorr.hip, order.hip, ergodic.hip, fan.hip, score.hip; the predictive mixture's LDS tile stands in mixture_tile.hpp):
// one copy of each, so that the next feature starts from parts and not from a paste.  Every piece is here in the form under
// which every kernel that uses it compiles to the device assembly it had with its own copy (DESIGN.md section 9,
// tools/isa_same.py); profiles/r10/README.md lists the forms that did not, and which copies stayed where they were.
// The macros are macros for that reason: as __forceinline__ functions the same statements compile to other code.
#pragma once
#include <hip/hip_runtime.h>

#include "round5.hpp"
#include "stat_plan.hpp"

namespace hmcg {

// One step omega <- omega A of the h-step weights omega = pi_end A^h: a row vector times the draw's transition matrix, k
// ascending in every dot product.  This is THE expression: the three features that weight the states by omega hold the same
// omega bits because they all expand it (tests/test_gpu_stat_omega.py compares them bit for bit).
// wv_: double[K_], updated in place; a_: column c of row i at a_[(i + K_ * c) * S_] -- S_ = 1 for a matrix in registers, the
// tile width for one staged in LDS by column with a_ pointing at the draw.
#define HMCG_OMEGA_STEP(K_, wv_, a_, S_)                                                                                  \
    do {                                                                                                                  \
        double nw_[K_];                                                                                                   \
        _Pragma("unroll") for (int c_ = 0; c_ < K_; ++c_) {                                                               \
            double t_ = wv_[0] * (a_)[(K_ * c_) * S_];                                                                    \
            _Pragma("unroll") for (int i_ = 1; i_ < K_; ++i_) t_ += wv_[i_] * (a_)[(i_ + K_ * c_) * S_];                  \
            nw_[c_] = t_;                                                                                                 \
        }                                                                                                                 \
        _Pragma("unroll") for (int c_ = 0; c_ < K_; ++c_) wv_[c_] = nw_[c_];                                              \
    } while (0)

// The sum of a double over the 64 lanes, in every lane: the fixed butterfly xor 32, 16, .. 1.
#define HMCG_WAVE_SUM(t_)                                                                                                 \
    do {                                                                                                                  \
        _Pragma("unroll") for (int m_ = 32; m_ >= 1; m_ >>= 1) t_ += __shfl_xor(t_, m_, 64);                              \
    } while (0)

// A draw value as the statistics read it: rounded as a CSV cell is when the call asks for it.
__device__ __forceinline__ double stat_in(double x, int r5) { return r5 ? round5(x) : x; }

__device__ __forceinline__ double stat_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// Thread tid's draw of tile `it` (nt draws) of the slab [dbeg, dend) as a wave-uniform 64-bit base and a 32-bit lane offset:
// every column is one scalar-base load, no 64-bit address per column.  it < 0: a pivot pass, thread 0 on the window's draw 0.
struct StatTile { size_t base; unsigned o; bool valid; };
__device__ __forceinline__ StatTile stat_tile(int it, int nt, int tid, long long dbeg, long long dend)
{
    StatTile t;
    t.base = it < 0 ? (size_t)0 : (size_t)dbeg;
    t.o = it < 0 ? 0u : (unsigned)(it * nt + tid);
    t.valid = it < 0 ? tid == 0 : (long long)t.base + t.o < dend;
    return t;
}

}  // namespace hmcg

// Block blockIdx.x of a launch of nslab_ slabs per window over nd_ draws: declares its window w_, its slab s_ and the slab's
// draws [dbeg_, dend_).
#define HMCG_STAT_SLAB(w_, s_, dbeg_, dend_, nslab_, nd_)                                                                 \
    const int w_ = (int)((long long)blockIdx.x / (nslab_));                                                               \
    const long long s_ = (long long)blockIdx.x - (long long)w_ * (nslab_);                                                \
    const long long dbeg_ = s_ * hmcg_host::PRED_SLAB;                                                                    \
    const long long dend_ = dbeg_ + hmcg_host::PRED_SLAB < (nd_) ? dbeg_ + hmcg_host::PRED_SLAB : (nd_)

// The slab sums of a launch: the offset of row (window w_, slab slab_ of the run's total_) of items_ doubles ...
#define HMCG_STAT_ROW(w_, total_, slab_, items_) (((size_t)(w_) * (size_t)(total_) + (size_t)(slab_)) * (size_t)(items_))
// ... and one item's sum over the slabs, in slab order: declares sum_ (col_: the item in slab 0, stride_: doubles between
// two slabs).
#define HMCG_SLAB_SUM(sum_, col_, nslab_, stride_)                                                                        \
    double sum_ = 0.0;                                                                                                    \
    for (long long sl_ = 0; sl_ < (nslab_); ++sl_) sum_ += (col_)[(size_t)sl_ * (size_t)(stride_)]

// Host: a kernel template instantiated for every K = 2..HMCG_MAXK; LAUNCH_(K) is the statement that launches one.
static_assert(HMCG_MAXK == 8, "HMCG_SWITCH_K lists the cases");
#define HMCG_SWITCH_K(k_, LAUNCH_)                                                                                        \
    switch (k_) {                                                                                                         \
        case 2: LAUNCH_(2); break;                                                                                        \
        case 3: LAUNCH_(3); break;                                                                                        \
        case 4: LAUNCH_(4); break;                                                                                        \
        case 5: LAUNCH_(5); break;                                                                                        \
        case 6: LAUNCH_(6); break;                                                                                        \
        case 7: LAUNCH_(7); break;                                                                                        \
        case 8: LAUNCH_(8); break;                                                                                        \
        default: return hipErrorInvalidValue;                                                                             \
    }
// Host: launch kernel_ (one instance of a template) with lds_ bytes of dynamic LDS, raising the kernel's limit to that first.
#define HMCG_LAUNCH_LDS(kernel_, grid_, block_, lds_, stream_, p_)                                                        \
    do {                                                                                                                  \
        hipError_t e_ = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel_), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds_)); \
        if (e_ != hipSuccess) return e_;                                                                                  \
        hipLaunchKernelGGL(kernel_, grid_, block_, lds_, stream_, p_);                                                    \
    } while (0)
