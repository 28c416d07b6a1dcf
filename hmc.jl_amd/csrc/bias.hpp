// bias.hpp -- host-side launchers of the uncertainty-bias moment kernels (bias.hip): mean and covariance over a window's draws
// of [pi_end A^h | mu] and the two numbers code/hassan_cdfs/bias_calcs.jl:40-53 reduces them to.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "bias_plan.hpp"

namespace hmcg_host {

struct BiasArgs {
    const double* mu; const double* pi_end; const double* A;   // device draw arrays (A: NULL when horizon is 0)
    const double* fc;          // device, the forecast-error column of window 0 (NULL: none); window w's lies fc_wstride doubles further
    long long fc_wstride;
    double* part;              // device, bias_part_doubles(): [W][nslab_total][items] slab sums, then [W][2K + 1] pivots
    long long nd, nd_ld;       // draws in this block (a whole number of slabs unless it ends the run) and the arrays' leading dimension
    long long slab0, nslab_total;      // this block's first slab among the run's
    int W, K, horizon;
    bool round5;
};
size_t bias_part_doubles(int W, long long nd, int K);
hipError_t launch_bias(const BiasArgs& a, hipStream_t stream);
// out[w] = uncbias, totalbias, mean[2K], cov[2K][2K] from the window's slab sums, added in slab order
hipError_t launch_bias_finalize(const double* part, double* out, int W, int K, long long nd_total, bool with_fc, hipStream_t stream);

}  // namespace hmcg_host
