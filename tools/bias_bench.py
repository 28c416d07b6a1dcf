"""Timing of the uncertainty-bias device entry at the production shape, for the record (no threshold).

  python tools/bias_bench.py [--W 460] [--nd 250000] [--K 3] [--horizon 12] [--reps 7] [--out profiles/bias_moments_timing.txt]

Prints (and with --out writes): the HIP-event time of hmcg_bias_moments_device (median of --reps after a warm-up; draws generated
on the device), the bytes the call reads -- 8 (2K + K^2 + 1) per draw: mu, pi_end, A and the forecast-error column -- and that
byte count over the HBM rate a streaming read achieves on this part, 6.3 TB/s (measured; DESIGN.md section 4 uses the same
figure as `frac_of_achievable`), beside the nominal 8 TB/s."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_ACHIEVABLE = 6.3e12        # B/s: a streaming read as measured on an MI355X (79 % of the nominal rate)
HBM_NOMINAL = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--W", type=int, default=460)
    ap.add_argument("--nd", type=int, default=250000)
    ap.add_argument("--K", type=int, default=3)
    ap.add_argument("--horizon", type=int, default=12)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from hmc_jl_amd import _lib
    _lib.load()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    W, K, nd, h = a.W, a.K, a.nd, a.horizon
    f64 = dict(generator=g, device=dev, dtype=torch.float64)
    mu = torch.randn((W, K, nd), **f64) * 3.0 + 2.0
    pi = torch.rand((W, K, nd), **f64) + 0.01
    pi /= pi.sum(dim=1, keepdim=True)
    A = torch.rand((W, K, K, nd), **f64) + 0.01          # A[w, j, i, d]: row i sums to 1 over j
    A /= A.sum(dim=1, keepdim=True)
    fc = torch.randn((W, 2, nd), **f64)
    out = torch.empty((W, _lib.bias_stride(K)), device=dev, dtype=torch.float64)
    torch.cuda.synchronize(dev)
    b = _lib.make_bias(W, K, nd, nd, h, 1, 0, True)
    times = []
    for rep in range(a.reps + 1):
        tm = _lib.bias_moments_device(b, mu.data_ptr(), pi.data_ptr(), A.data_ptr() if h > 0 else 0, fc.data_ptr(), out.data_ptr(), None, True)
        if rep:
            times.append(tm.kernel_ms)
    ms = statistics.median(times)
    nbytes = 8.0 * (2 * K + (K * K if h > 0 else 0) + 1) * W * nd
    t_ach, t_nom = nbytes / HBM_ACHIEVABLE * 1e3, nbytes / HBM_NOMINAL * 1e3
    o = _lib.unpack_bias(out.cpu().numpy(), K)
    lines = [
        "Uncertainty-bias moments (hmcg_bias_moments_device), one MI355X -- for the record, no threshold.",
        "tools/bias_bench.py: W = %d windows, nd = %d draws, K = %d, horizon %d, round5 on, fcast given (H = 1); draws generated on the"
        % (W, nd, K, h),
        "device; HIP events around the two kernels; median of %d timed calls after one warm-up call." % len(times),
        "",
        "  device entry, all %d windows          %.3f ms   (min %.3f, max %.3f)" % (W, ms, min(times), max(times)),
        "  bytes read                             %.3f GB   (8 (2K + K^2 + 1) = %d B per draw)" % (nbytes / 1e9, nbytes / W / nd),
        "  bytes / 6.3 TB/s (measured achievable) %.3f ms   -> device / that = %.2f, %.2f TB/s achieved" % (t_ach, ms / t_ach, nbytes / ms / 1e9),
        "  bytes / 8 TB/s (nominal)               %.3f ms   -> device / that = %.2f" % (t_nom, ms / t_nom),
        "  results finite                         %s" % all(bool(np.isfinite(v).all()) for v in o.values()),
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
