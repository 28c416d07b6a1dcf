// order.hpp -- host-side launcher of the selection kernel (order.hip): per draw column the exact quantiles of a list of
// probabilities, their bracketing order statistics and the NaN count (include/hmcg_order.h: hmcg_chain_quantiles).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "order_plan.hpp"

namespace hmcg_host {

struct OrdArgs {
    const double* x;           // device: column b of this launch at x + ld * b, nd draws each
    double* q;                 // device [ncols][Q][HMCG_ORD_STRIDE], of this launch's first column
    int64_t* n;                // device [ncols][2]
    long long ncols, nd, ld;   // columns of this launch (one block each); draws per column; leading dimension of x
    int Q;
    bool round5;
    double probs[HMCG_ORD_MAXQ];
};
int ord_lds_bytes();
hipError_t launch_chain_quantiles(const OrdArgs& a, hipStream_t stream);

}  // namespace hmcg_host
