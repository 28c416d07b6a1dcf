// HBM-streaming forms of the LDS-resident kernel WITH the smoothing pass: plain and signal path
#include <hip/hip_runtime.h>
#include "variants.hpp"
#include "gibbs_big.hpp"
namespace hmcg_host {
const BigForm g_big_011 = HMCG_BIG_FORM(false, true, true);
const BigForm g_big_111 = HMCG_BIG_FORM(true, true, true);
}
