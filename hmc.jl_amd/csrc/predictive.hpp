// predictive.hpp -- host-side launchers of the predictive-CDF kernels (predictive.hip): the draw mean of the regime mixture's
// normal CDF on a grid (code/hassan_cdfs/calc_cdfs.jl:39-41), per window and horizon.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "predictive_plan.hpp"

namespace hmcg_host {

struct PredictiveArgs {
    const double* mu; const double* sig2; const double* pi_end; const double* A;   // device draw arrays (A: NULL when every horizon is 0)
    const double* grid;        // device, [G]
    double* part;              // device, [W][nslab_total][n_h * G]: slab sums
    long long nd, nd_ld;       // draws in this block (a whole number of slabs unless it ends the run) and the arrays' leading dimension
    long long slab0, nslab_total;      // this block's first slab among the run's
    int W, K, G, n_h;
    int horizons[HMCG_MAXH];
    bool round5;
};
size_t predictive_part_doubles(int W, long long nd, int n_h, int G);
hipError_t launch_predictive(const PredictiveArgs& a, hipStream_t stream);
// cdf[w][j][g] = (sum of the window's slab sums, in slab order) / nd_total
hipError_t launch_predictive_finalize(const double* part, double* cdf, int W, int n_h, int G, long long nd_total, hipStream_t stream);

}  // namespace hmcg_host
