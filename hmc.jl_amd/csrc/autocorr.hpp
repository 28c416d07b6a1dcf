// autocorr.hpp -- host-side launchers of the autocorrelation kernels (autocorr.hip): per window and draw column the
// autocovariances up to lag L, Geyer's integrated autocorrelation time, effective sample size, Monte-Carlo standard error and
// split-R-hat (include/hmcg.h: hmcg_chain_autocorr).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "autocorr_plan.hpp"

namespace hmcg_host {

// Work area of a call, device memory: per (window, column) L + 1 running lag sums | 6 running sums | pivot | [2][L] edge values.
size_t acf_work_bytes(int W, int C, int L);

struct AcfArgs {
    const double* x;           // device draw array of this block: draw d of the run, column c, window w at (d - d_origin + pre) + ld * (c + C * w)
    void* work;                // device, acf_work_bytes()
    double* acov;              // device [W][C][L + 1]
    double* diag;              // device [W][C][HMCG_ACF_STRIDE]
    long long d_origin, n;     // this block owns draws [d_origin, d_origin + n) of the run; d_origin is a slab boundary
    long long pre;             // draws in front of d_origin that x holds as well: acf_pre(d_origin, L)
    long long nd, ld;          // draws of the whole run; leading dimension of x
    int W, C, L;
    bool round5;
};
// lag sums, S1 / S2 and edge values of this block's slabs into the work area (the block with d_origin == 0 starts them)
hipError_t launch_autocorr_accumulate(const AcfArgs& a, hipStream_t stream);
// acov and diag from the work area, after the last block
hipError_t launch_autocorr_finalize(const AcfArgs& a, hipStream_t stream);

}  // namespace hmcg_host
