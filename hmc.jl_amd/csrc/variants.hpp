// variants.hpp -- how the variants_*.hip units fill the tables of compiled kernel instantiations (plan.hpp): the macros that
// name the kernel templates.  The rows are split over several translation units so that they compile in parallel; hmcg.hip
// only sees the tables.
#pragma once
#include "gibbs_device.hpp"
#include "plan.hpp"

namespace hmcg_host {

#define HMCG_BIG(K_, SIG_, SM_, ST_) { K_, 256, hmcg::gibbs_sweeps_kernel_big<K_, 256, SM_, ST_, SIG_> }
#define HMCG_BIG_FORM(SIG_, SM_, ST_)                                                                                \
    { HMCG_BIG(2, SIG_, SM_, ST_), HMCG_BIG(3, SIG_, SM_, ST_), HMCG_BIG(4, SIG_, SM_, ST_), HMCG_BIG(5, SIG_, SM_, ST_), \
      HMCG_BIG(6, SIG_, SM_, ST_), HMCG_BIG(7, SIG_, SM_, ST_), HMCG_BIG(8, SIG_, SM_, ST_) }

#define HMCG_V(K_, L_, NT_, SIG_, SM_, NH_, OCC_, PS_, PB_) \
    { K_, L_, NT_, hmcg::gibbs_sweeps_kernel<K_, L_, NT_, SIG_, SM_, NH_, OCC_>, SIG_, SM_, NH_, OCC_, PS_, PB_ }
// every 256-thread variant in the three flavours, with the one to prefer for small and for large batches
// (measured: tools/variant_sweep.py, profiles/r01/variant_sweep.txt -- helper waves win while they fit the
// 256-register cap without spilling, capped plain blocks win once two windows can share a CU)
#define HMCG_V3(K_, L_, SIG_, SM_, PS_, PB_)                                                   \
    HMCG_V(K_, L_, 256, SIG_, SM_, 0, 1, PS_, PB_), HMCG_V(K_, L_, 256, SIG_, SM_, 0, 2, PS_, PB_), \
    HMCG_V(K_, L_, 256, SIG_, SM_, 4, 2, PS_, PB_)
#define HMCG_GROUP(name_, array_) const VariantGroup name_ = { array_, (int)(sizeof(array_) / sizeof(array_[0])) }

}  // namespace hmcg_host
