// LDS-resident kernels: K = 5..8, and K = 2..4 for windows too long for the register-resident variants
#include <hip/hip_runtime.h>
#include "variants.hpp"
#include "gibbs_big.hpp"
namespace hmcg_host {
const BigForm g_big_000 = HMCG_BIG_FORM(false, false, false);
// ... with the backward pass every kept sweep (smoothed / filtered probability means streamed through HBM)
const BigForm g_big_010 = HMCG_BIG_FORM(false, true, false);
const BigForm* const g_big[2][2][2] = { { { &g_big_000, &g_big_001 }, { &g_big_010, &g_big_011 } },
                                        { { &g_big_100, &g_big_101 }, { &g_big_110, &g_big_111 } } };
}
