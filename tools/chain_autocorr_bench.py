"""Timing of the autocorrelation device entry at the production shape, for the record (no threshold).

  python tools/chain_autocorr_bench.py [--W 460] [--nd 250000] [--reps 7] [--out profiles/chain_autocorr_timing.txt]

Prints (and with --out writes): the HIP-event time of hmcg_chain_autocorr_device (median of --reps after a warm-up, with the
spread; AR(1) draws generated on the device) at C = 3 and 9 columns and L = 255 and 1023 lags; beside each the floor of its
arithmetic -- W C nd (L + 1) fp64 FMAs at one 64-lane FMA per 4.03 cycles and SIMD (measured), 1024 SIMDs,
2.4 GHz -- and the ratio to it.  In the same session hmcg_mixture_moments_device at its recorded shape (K = 3, horizons
(0, 12)) as the yardstick."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FMA_PER_S = 1024 * 64 / 4.03 * 2.4e9       # fp64 vector FMAs per second of the whole chip at the largest clock


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--W", type=int, default=460)
    ap.add_argument("--nd", type=int, default=250000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from hmc_jl_amd import _lib
    _lib.load()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    W, nd = a.W, a.nd
    f64 = dict(generator=g, device=dev, dtype=torch.float64)

    def median_ms(call):
        times = []
        for rep in range(a.reps + 1):
            tm = call()
            if rep:
                times.append(tm.kernel_ms)
        return statistics.median(times), min(times), max(times)

    lines = ["Autocorrelation, effective sample size and split-R-hat (hmcg_chain_autocorr_device), one MI355X -- for the record, no threshold.",
             "tools/chain_autocorr_bench.py: W = %d windows, nd = %d draws, round5 on; draws generated on the device (a moving average of"
             % (W, nd),
             "eight normals about a centre per column, so neighbouring draws correlate); HIP events around the two kernels; median of %d"
             % a.reps,
             "timed calls after one warm-up call.  Floor: W C nd (L + 1) fp64 FMAs at %.1f T FMA/s (one 64-lane FMA per 4.03 cycles"
             % (FMA_PER_S / 1e12),
             "and SIMD, 1024 SIMDs, 2.4 GHz).", ""]
    for Cn in (3, 9):
        e = torch.randn((W, Cn, nd + 7), **f64)
        x = e.unfold(2, 8, 1).mean(dim=3) * 0.8 + torch.randn((W, Cn, 1), **f64) * 2.0 + 3.0
        x = x.contiguous()
        del e
        for L in (255, 1023):
            acov = torch.empty((W, Cn, L + 1), device=dev, dtype=torch.float64)
            diag = torch.empty((W, Cn, _lib.ACF_STRIDE), device=dev, dtype=torch.float64)
            torch.cuda.synchronize(dev)
            p = _lib.make_autocorr(W, Cn, nd, nd, L, 0, True)
            ms, lo, hi = median_ms(lambda: _lib.chain_autocorr_device(p, x.data_ptr(), acov.data_ptr(), diag.data_ptr(), None, True))
            fmas = float(W) * Cn * nd * (L + 1)
            floor = fmas / FMA_PER_S * 1e3
            d = diag.cpu().numpy()
            lines.append("  C = %d, L = %4d  %9.3f ms   (min %.3f, max %.3f)   %.3e FMAs, floor %.3f ms, x %.2f of it; %.2f T FMA/s"
                         % (Cn, L, ms, lo, hi, fmas, floor, ms / floor, fmas / ms / 1e9))
            lines.append("      results finite: %s; tau median %.2f, ess median %.0f, truncated %d of %d, rhat max %.4f"
                         % (bool(np.isfinite(acov.cpu().numpy()).all() and np.isfinite(d).all()), float(np.median(d[..., 2])),
                            float(np.median(d[..., 3])), int(d[..., 6].sum()), d[..., 6].size, float(d[..., 7].max())))
            del acov, diag
        del x
    K, hz = 3, (0, 12)
    mu = torch.randn((W, K, nd), **f64) * 3.0 + 2.0
    sig2 = torch.rand((W, K, nd), **f64) * 2.0 + 0.05
    pi = torch.rand((W, K, nd), **f64) + 0.01
    pi /= pi.sum(dim=1, keepdim=True)
    A = torch.rand((W, K, K, nd), **f64) + 0.01
    A /= A.sum(dim=1, keepdim=True)
    out = torch.empty((W, len(hz), _lib.MIX_STRIDE), device=dev, dtype=torch.float64)
    torch.cuda.synchronize(dev)
    mp = _lib.make_mixmom(W, K, nd, nd, hz, 0, True)
    ms, lo, hi = median_ms(lambda: _lib.mixture_moments_device(mp, mu.data_ptr(), sig2.data_ptr(), pi.data_ptr(), A.data_ptr(), out.data_ptr(), None, True))
    mbytes = 8.0 * (3 * K + K * K) * W * nd
    lines += ["", "  hmcg_mixture_moments_device, K = 3, horizons [0, 12], same W and nd, same session:",
              "    %-28s %8.3f ms   (min %.3f, max %.3f)   %.3f GB read, %.2f TB/s" % ("yardstick", ms, lo, hi, mbytes / 1e9, mbytes / ms / 1e9)]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
