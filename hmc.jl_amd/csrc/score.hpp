// score.hpp -- host-side launchers of the predictive-score kernels (score.hip): CRPS, PIT and density of the regime mixture
// against the realised value, per window and horizon (include/hmcg_score.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "score_plan.hpp"

namespace hmcg_host {

struct ScoreArgs {
    const double* mu; const double* sig2; const double* pi_end; const double* A;   // device draw arrays (A: NULL when every horizon is 0)
    const double* yreal;       // device, [n_h][yreal_ld]; this launch's windows begin at column w0
    double* work;              // device, [W][score_work(n_u, K, n_h).total]
    double* out;               // device, [W][n_h][5] of this launch's windows
    long long n_u, stride, nd_ld;      // used draws, their distance in the draw arrays, the arrays' leading dimension
    long long yreal_ld, w0;
    int W, K, n_h;
    int horizons[HMCG_MAXH];
    bool round5;
};
size_t score_lds_bytes(int K, int n_h, bool with_A);
// the components and weights into the work area, and the slab sums of F, E, P at yreal ...
hipError_t launch_score_components(const ScoreArgs& a, hipStream_t stream);
// ... the pair sums, one partial per (window, block, horizon) ...
hipError_t launch_score_pairs(const ScoreArgs& a, hipStream_t stream);
// ... and out from the slab sums and the partials
hipError_t launch_score_finish(const ScoreArgs& a, hipStream_t stream);

}  // namespace hmcg_host
