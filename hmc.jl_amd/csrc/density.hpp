// density.hpp -- host-side launchers of the chain-density kernels (density.hip): per window and draw column the binned counts of
// nested prefixes of the chain, their mean and variance, and the running mean (plots/mcplots.jl, plots/timeseriesplots.jl up
// to the drawing).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "density_plan.hpp"

namespace hmcg_host {

// Work area of a call, device memory: [W][pieces][C][3] piece sums S1, S2 and the S1 before the piece | [W][C] pivots | [W][C][2] range keys (64-bit).
size_t dens_work_bytes(int W, int C, long long nd, const int64_t* cuts, int n_cuts);

struct DensArgs {
    const double* x;           // device draw array of this block: element (d, c, w) of the run at (d - d_origin) + nd_ld * (c + C * w)
    void* work;                // device, dens_work_bytes()
    double* range;             // device [W][C][2]
    unsigned long long* counts;        // device [W][C][n_cuts][B + 3]: per-segment counts until the finalize kernel has run
    double* stats;             // device [W][C][n_cuts][2]
    double* trace;             // device [W][C][trace_len] (unused with trace_len == 0)
    long long d_origin, n;     // this block holds draws [d_origin, d_origin + n) of the run; d_origin is a slab boundary
    long long nd, nd_ld;       // draws of the whole run; leading dimension of x
    long long trace_stride;
    int64_t cuts[HMCG_MAXH];
    int W, C, B, n_cuts, trace_len;
    bool round5;
};
// range keys to "nothing seen", counts to zero: once per call, before anything else
hipError_t launch_density_clear(const DensArgs& a, hipStream_t stream);
// min / max of the finite x' of this block's draws into the range keys
hipError_t launch_density_range(const DensArgs& a, hipStream_t stream);
// range[w][c] = lo_hi[w][c] (device memory) when given, else the decoded keys
hipError_t launch_density_resolve(const DensArgs& a, const double* lo_hi, hipStream_t stream);
// counts per segment, piece sums and in-piece trace sums of this block's pieces below the last cut (needs `range`)
hipError_t launch_density_accumulate(const DensArgs& a, hipStream_t stream);
// nested prefix counts, stats at every cut, trace points
hipError_t launch_density_finalize(const DensArgs& a, hipStream_t stream);

}  // namespace hmcg_host
