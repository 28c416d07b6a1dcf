// LDS-resident kernel on the signal Monte-Carlo path (estimatesignals!, src/Hmc.jl:868-914): K = 5..8, and K = 2..4 for windows
// too long for the register-resident SIG variants; LDS-resident and HBM-streaming forms
#include <hip/hip_runtime.h>
#include "variants.hpp"
#include "gibbs_big.hpp"
namespace hmcg_host {
const BigForm g_big_100 = HMCG_BIG_FORM(true, false, false);
const BigForm g_big_101 = HMCG_BIG_FORM(true, false, true);
// ... with the smoothing pass (K <= 4 within the register-resident range run variants_sigsmooth.hip instead)
const BigForm g_big_110 = HMCG_BIG_FORM(true, true, false);
}
