"""Timing of the predictive-quantile device entry at the production shape, for the record (no threshold).

  python tools/fan_bench.py [--W 460] [--nd 250000] [--reps 7] [--rounds 4] [--K 3 8] [--h0-only] [--out profiles/fan_timing.txt]

For K = 3 and K = 8 and the horizons (0,) and (0, 12), with the fan-chart probabilities (0.025, 0.16, 0.5, 0.84, 0.975): the
HIP-event time of hmcg_predictive_quantiles_device (median of --reps after a warm-up; draws generated on the device) and, as
the yardstick, hmcg_predictive_cdf_device in the same session on the same draws and horizons with G = 81 grid points.  Both
are counted in Phi evaluations -- W nd K n_h (129 + (R - 1) n_p 31) against W nd K n_h G -- and the ratio of the two Phi rates
is written down beside the total time.  The text goes to --out as well as to the terminal."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROBS = (0.025, 0.16, 0.5, 0.84, 0.975)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--W", type=int, default=460)
    ap.add_argument("--nd", type=int, default=250000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--G", type=int, default=81)
    ap.add_argument("--K", type=int, nargs="+", default=[3, 8])
    ap.add_argument("--h0-only", action="store_true", help="horizons (0,) alone (a profiler run of one shape)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fan_timing.txt"))
    a = ap.parse_args()
    import torch
    from hmc_jl_amd import _lib
    _lib.load()
    dev = torch.device("cuda", 0)
    W, nd, R, G = a.W, a.nd, a.rounds, a.G
    lines = ["Predictive quantiles (hmcg_predictive_quantiles_device), production shape, one MI355X -- for the record, no threshold.",
             "tools/fan_bench.py: W = %d windows, nd = %d draws, probabilities %s, %d rounds, round5 on; draws generated on the" % (W, nd, PROBS, R),
             "device; HIP events around the %d kernels of a call; median of %d timed calls after one warm-up call.  Yardstick:" % (2 + 2 * R, a.reps),
             "hmcg_predictive_cdf_device in the same session on the same draws and horizons, G = %d.  Phi: evaluations of the normal CDF." % G,
             ""]

    def median_ms(call):
        times = []
        for rep in range(a.reps + 1):
            tm = call()
            if rep:
                times.append(tm.kernel_ms)
        return statistics.median(times), min(times), max(times)

    grid = torch.from_numpy(np.linspace(-5.0, 15.0, G)).to(dev)
    for K in a.K:
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        mu = torch.randn((W, K, nd), generator=g, device=dev, dtype=torch.float64) * 3.0 + 2.0
        sig2 = torch.rand((W, K, nd), generator=g, device=dev, dtype=torch.float64) * 4.0 + 0.05
        pi = torch.rand((W, K, nd), generator=g, device=dev, dtype=torch.float64) + 0.01
        pi /= pi.sum(dim=1, keepdim=True)
        A = None
        for hz in ((0,),) if a.h0_only else ((0,), (0, 12)):
            if max(hz) > 0 and A is None:
                A = torch.rand((W, K, K, nd), generator=g, device=dev, dtype=torch.float64) + 0.01
                A /= A.sum(dim=1, keepdim=True)             # A[w, j, i, d]: row i sums to 1 over j
            dA = A.data_ptr() if max(hz) > 0 else 0
            n_h, n_p = len(hz), len(PROBS)
            out = torch.empty((W, n_h, n_p, _lib.FAN_STRIDE), device=dev, dtype=torch.float64)
            rng = torch.empty((W, 2), device=dev, dtype=torch.float64)
            flag = torch.empty((W, n_h, n_p), device=dev, dtype=torch.int32)
            cdf = torch.empty((W, n_h, G), device=dev, dtype=torch.float64)
            torch.cuda.synchronize(dev)
            fan = _lib.make_fan(W, K, nd, nd, PROBS, hz, R, 0, True)
            pred = _lib.make_predictive(W, K, nd, nd, G, hz, 0, True)
            f_ms, f_lo, f_hi = median_ms(lambda: _lib.predictive_quantiles_device(fan, mu.data_ptr(), sig2.data_ptr(), pi.data_ptr(), dA,
                                                                                  out.data_ptr(), rng.data_ptr(), flag.data_ptr(), None, True))
            c_ms, c_lo, c_hi = median_ms(lambda: _lib.predictive_cdf_device(pred, mu.data_ptr(), sig2.data_ptr(), pi.data_ptr(), dA,
                                                                            grid.data_ptr(), cdf.data_ptr(), None, True))
            f_phi = float(W) * nd * K * n_h * (129 + (R - 1) * n_p * 31)
            c_phi = float(W) * nd * K * n_h * G
            f_rate, c_rate = f_phi / (f_ms * 1e-3), c_phi / (c_ms * 1e-3)
            fl = flag.cpu().numpy()
            lines += ["K = %d, horizons %s" % (K, hz),
                      "  quantile entry   %9.2f ms   (min %.2f, max %.2f; %.3e Phi, %.3e Phi/s; flags %s)" % (f_ms, f_lo, f_hi, f_phi, f_rate, np.unique(fl)),
                      "  CDF entry        %9.2f ms   (min %.2f, max %.2f; %.3e Phi, %.3e Phi/s)" % (c_ms, c_lo, c_hi, c_phi, c_rate),
                      "  Phi rate, quantile entry / CDF entry   %.2f;   time in CDF calls   %.2f (from the Phi count alone: %.2f)"
                      % (f_rate / c_rate, f_ms / c_ms, f_phi / c_phi),
                      ""]
            print("\n".join(lines[-5:]), flush=True)
            del out, rng, flag, cdf
        del mu, sig2, pi, A
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    with open(a.out, "w") as fh:
        fh.write(text)
    print("written to %s" % a.out)


if __name__ == "__main__":
    main()
