"""Timing of the predictive-mixture moment device entry at the production shape, for the record (no threshold).

  python tools/mixmoments_bench.py [--W 460] [--nd 250000] [--K 3] [--horizons 0,12] [--reps 7] [--out profiles/mixture_moments_timing.txt]

Prints (and with --out writes): the HIP-event time of hmcg_mixture_moments_device (median of --reps after a warm-up; draws
generated on the device), the bytes the call reads -- 8 (3K + K^2) per draw: mu, sig2, pi_end and A -- and that byte count
over the HBM rate a streaming read achieves on this part, 6.3 TB/s (measured; DESIGN.md section 4 uses the same figure as
`frac_of_achievable`), beside the nominal 8 TB/s.  With --bias-ms (the median tools/bias_bench.py reports at the same W, nd, K
in the same session) also the ratio of the two kernels' time per byte."""
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
    ap.add_argument("--horizons", default="0,12")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--bias-ms", type=float, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from hmc_jl_amd import _lib
    _lib.load()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    W, K, nd = a.W, a.K, a.nd
    hz = tuple(int(h) for h in a.horizons.split(","))
    with_A = any(h > 0 for h in hz)
    f64 = dict(generator=g, device=dev, dtype=torch.float64)
    mu = torch.randn((W, K, nd), **f64) * 3.0 + 2.0
    sig2 = torch.rand((W, K, nd), **f64) * 2.0 + 0.05
    pi = torch.rand((W, K, nd), **f64) + 0.01
    pi /= pi.sum(dim=1, keepdim=True)
    A = torch.rand((W, K, K, nd), **f64) + 0.01          # A[w, j, i, d]: row i sums to 1 over j
    A /= A.sum(dim=1, keepdim=True)
    out = torch.empty((W, len(hz), _lib.MIX_STRIDE), device=dev, dtype=torch.float64)
    torch.cuda.synchronize(dev)
    p = _lib.make_mixmom(W, K, nd, nd, hz, 0, True)
    times = []
    for rep in range(a.reps + 1):
        tm = _lib.mixture_moments_device(p, mu.data_ptr(), sig2.data_ptr(), pi.data_ptr(), A.data_ptr() if with_A else 0, out.data_ptr(), None, True)
        if rep:
            times.append(tm.kernel_ms)
    ms = statistics.median(times)
    per_draw = 8.0 * (3 * K + (K * K if with_A else 0))
    nbytes = per_draw * W * nd
    t_ach, t_nom = nbytes / HBM_ACHIEVABLE * 1e3, nbytes / HBM_NOMINAL * 1e3
    o = _lib.unpack_mixture_moments(out.cpu().numpy())
    lines = [
        "Predictive-mixture moments (hmcg_mixture_moments_device), one MI355X -- for the record, no threshold.",
        "tools/mixmoments_bench.py: W = %d windows, nd = %d draws, K = %d, horizons %s, round5 on; draws generated on the device;"
        % (W, nd, K, list(hz)),
        "HIP events around the two kernels; median of %d timed calls after one warm-up call." % len(times),
        "",
        "  device entry, all %d windows          %.3f ms   (min %.3f, max %.3f)" % (W, ms, min(times), max(times)),
        "  bytes read                             %.3f GB   (8 (3K + K^2) = %d B per draw)" % (nbytes / 1e9, per_draw),
        "  bytes / 6.3 TB/s (measured achievable) %.3f ms   -> device / that = %.2f, %.2f TB/s achieved" % (t_ach, ms / t_ach, nbytes / ms / 1e9),
        "  bytes / 8 TB/s (nominal)               %.3f ms   -> device / that = %.2f" % (t_nom, ms / t_nom),
    ]
    if a.bias_ms is not None:
        bias_bytes = 8.0 * (2 * K + K * K + 1) * W * nd
        lines.append("  hmcg_bias_moments_device, same shape   %.3f ms   (%d B per draw, tools/bias_bench.py in the same session)"
                     % (a.bias_ms, bias_bytes / W / nd))
        lines.append("  time ratio %.2f; time per byte ratio   %.2f" % (ms / a.bias_ms, (ms / nbytes) / (a.bias_ms / bias_bytes)))
    lines.append("  results finite                         %s" % all(bool(np.isfinite(v).all()) for v in o.values()))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
