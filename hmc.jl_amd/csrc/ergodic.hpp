// ergodic.hpp -- host-side launchers of the ergodic-moment kernels (ergodic.hip): per draw the stationary regime law, the
// expected durations and the long-run mean and variance; per window their mean and variance over the good draws.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "ergodic_plan.hpp"

namespace hmcg_host {

struct ErgArgs {
    const double* mu; const double* sig2; const double* A;     // device draw arrays
    double* cols;              // device, [W][C][nd_ld] per-draw columns of this block's draws (NULL: not kept)
    double* part;              // device, erg_part_doubles(): [W][nslab_total][items] slab sums, then [W][C] pivots
    long long nd, nd_ld;       // draws in this block (a whole number of slabs unless it ends the run) and the arrays' leading dimension
    long long slab0, nslab_total;      // this block's first slab among the run's
    int W, K;
    bool round5;
};
hipError_t launch_ergodic(const ErgArgs& a, hipStream_t stream);
// out[w][c] = (mean, variance) over the good draws and n[w] = (good, nd_total - good) from the window's slab sums, added in slab order
hipError_t launch_ergodic_finalize(const double* part, double* out, long long* n, int W, int K, long long nd_total, hipStream_t stream);

}  // namespace hmcg_host
