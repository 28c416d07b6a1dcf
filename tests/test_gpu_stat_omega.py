"""The three draw statistics that weight the states by omega = pi_end A^h -- predictive CDFs, bias moments, mixture moments --
build omega by one expression (HMCG_OMEGA_STEP of csrc/stat_device.hpp), so they must hold the same omega bits.  With a single
draw none of them sums over draws, and each hands the sum of its omega back untouched:
  mixture moments  weight[w, 0] = (omega_0 + omega_1 + ...) / 1, added in ascending k;
  predictive CDF   at y = 1e6 every Phi is exactly 1: F = omega_0 * 1, then fma(omega_k, 1, F) in ascending k, / 1;
  bias moments     mean[w, :K] = pivot + 0 / 1 = omega itself; added here in ascending k in float64.
The three numbers are compared as bit patterns."""
import numpy as np
import pytest

import mixmoments_cases as mc


@pytest.mark.gpu
@pytest.mark.parametrize("round5", [True, False])
@pytest.mark.parametrize("h", [1, 12])
@pytest.mark.parametrize("K", list(range(2, 9)))
def test_one_draw_gives_the_same_omega_sum_in_all_three_features(hmclib, K, h, round5):
    from hmc_jl_amd import _lib
    W = 2
    mu, sig2, pi, A = mc.make_draws(100 * K + h, W, K, 1)
    weight = _lib.unpack_mixture_moments(_lib.mixture_moments_host(mu, sig2, pi, A, (h,), round5=round5))["weight"][:, 0]
    cdf = _lib.predictive_cdf_host(mu, sig2, pi, A, np.array([1e6]), (h,), round5=round5)[:, 0, 0]
    omega = _lib.unpack_bias(_lib.bias_moments_host(mu, pi, A, None, h, round5=round5), K)["mean"][:, :K]
    total = omega[:, 0].copy()
    for k in range(1, K):
        total = total + omega[:, k]
    got = {"mixture moments": weight, "predictive CDF": cdf, "bias moments": total}
    bits = {name: np.ascontiguousarray(v, dtype=np.float64).view(np.uint64) for name, v in got.items()}
    print("K = %d, h = %d, round5 = %s:" % (K, h, round5), {name: [hex(int(b)) for b in v] for name, v in bits.items()})
    assert (np.abs(weight - 1.0) < 1e-3).all()               # a sum of omega, not a zero that would compare equal too
    assert np.array_equal(bits["mixture moments"], bits["predictive CDF"])
    assert np.array_equal(bits["mixture moments"], bits["bias moments"])
