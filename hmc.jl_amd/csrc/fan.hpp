// fan.hpp -- host-side launchers of the predictive-quantile kernels (fan.hip): the regime mixture's CDF inverted at a list of
// probabilities by grid refinement, per window and horizon (include/hmcg_fan.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "fan_plan.hpp"

namespace hmcg_host {

struct FanArgs {
    const double* mu; const double* sig2; const double* pi_end; const double* A;   // device draw arrays (A: NULL when every horizon is 0)
    double* part;              // device, [W][nslab_total][fan_max_items]: slab sums; the range pass keeps (min, max) in a row's first two
    double* out;               // device, [W][n_h][n_p][5]: the bracket table between the rounds, the result after the last
    double* range;             // device, [W][2]
    int32_t* flag;             // device, [W][n_h][n_p]
    long long nd, nd_ld;       // draws in this block (a whole number of slabs unless it ends the run) and the arrays' leading dimension
    long long slab0, nslab_total;      // this block's first slab among the run's
    int W, K, n_h, n_p;
    int horizons[HMCG_MAXH];
    double probs[HMCG_FAN_MAXP];
    bool round5;
};
// per-slab min / max of mu -+ 40 sd over the block's draws, then range[w] = their fmin / fmax over the run's slabs
hipError_t launch_fan_range(const FanArgs& a, hipStream_t stream);
hipError_t launch_fan_range_finalize(const FanArgs& a, hipStream_t stream);
// the slab sums of F at the points of round `round` (1-based) over the block's draws ...
hipError_t launch_fan_eval(const FanArgs& a, int round, hipStream_t stream);
// ... and, once every block of the run has been through: F, the cell choice, the next bracket table; last: q and flag
hipError_t launch_fan_step(const FanArgs& a, int round, bool last, long long nd_total, hipStream_t stream);

}  // namespace hmcg_host
