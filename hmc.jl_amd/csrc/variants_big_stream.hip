// LDS-resident kernel's HBM-streaming form: the per-step arrays in a global scratch -- windows beyond what the CU's LDS holds
#include <hip/hip_runtime.h>
#include "variants.hpp"
#include "gibbs_big.hpp"
namespace hmcg_host {
const BigForm g_big_001 = HMCG_BIG_FORM(false, false, true);
}
