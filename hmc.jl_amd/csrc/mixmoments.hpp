// mixmoments.hpp -- host-side launchers of the predictive-mixture moment kernels (mixmoments.hip): pooled mean, variance,
// skewness and excess kurtosis over a window's draws of sum_k omega_k N(mu_k, sig2_k), omega = pi_end A^h, and the within- /
// between-draw split (code/skewness.jl, code/alt_forecasts.jl asked of the draws).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "mixmoments_plan.hpp"

namespace hmcg_host {

struct MixArgs {
    const double* mu; const double* sig2; const double* pi_end; const double* A;   // device draw arrays (A: NULL when every horizon is 0)
    double* part;              // device, mix_part_doubles(): [W][nslab_total][n_h][MIX_ITEMS] slab sums, then [W][n_h][MIX_PIVOTS]
    long long nd, nd_ld;       // draws in this block (a whole number of slabs unless it ends the run) and the arrays' leading dimension
    long long slab0, nslab_total;      // this block's first slab among the run's
    int W, K, n_h;
    MixWalk walk;              // mix_walk() of the call
    bool round5;
};
size_t mix_part_doubles(int W, long long nd, int n_h);
hipError_t launch_mixmoments(const MixArgs& a, hipStream_t stream);
// out[w][j][0..7] from the window's slab sums, added in slab order
hipError_t launch_mixmoments_finalize(const double* part, double* out, int W, int n_h, long long nd_total, hipStream_t stream);

}  // namespace hmcg_host
