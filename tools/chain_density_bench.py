"""Timing of the chain-density device entry at the production shape, for the record (no threshold).

  python tools/chain_density_bench.py [--W 460] [--nd 250000] [--reps 7] [--out profiles/chain_density_timing.txt]

Prints (and with --out writes): the HIP-event time of hmcg_chain_density_device (median of --reps after a warm-up; draws
generated on the device) at the main shape -- C = 3 columns, 64 bins, the four cuts of plots/mcplots.jl scaled to nd
(0.4, 0.6, 0.8, 1.0 of it), a running mean of 10 000 x 1 -- and at C = 9, 512 bins; with the automatic range (two passes over
the data: the range kernel, then the counts) and with a given one (one pass); the bytes each reads, 8 C nd W per pass, and the
rate.  In the same session hmcg_mixture_moments_device at its recorded shape (K = 3, horizons (0, 12), 144 B per draw) as the
yardstick, and the ratio of the two kernels' time per byte."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_ACHIEVABLE = 6.3e12        # B/s: a streaming read as measured on an MI355X (79 % of the nominal rate)


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
    cuts = tuple(sorted({max(1, nd * k // 5) for k in (2, 3, 4, 5)}))
    trace = (min(10000, nd), 1)

    def median_ms(call):
        times = []
        for rep in range(a.reps + 1):
            tm = call()
            if rep:
                times.append(tm.kernel_ms)
        return statistics.median(times), min(times), max(times)

    lines = ["Chain densities and running means (hmcg_chain_density_device), one MI355X -- for the record, no threshold.",
             "tools/chain_density_bench.py: W = %d windows, nd = %d draws, cuts %s, running mean %d x %d, round5 on; draws generated"
             % (W, nd, list(cuts), trace[0], trace[1]),
             "on the device (clustered: a narrow normal about a centre per column); HIP events around the kernels; median of %d timed"
             % a.reps,
             "calls after one warm-up call.  Bytes read: 8 C nd W per pass over the data.", ""]
    per_byte = None
    for Cn, bins in ((3, 64), (9, 512)):
        x = torch.randn((W, Cn, nd), **f64) * 0.3 + torch.randn((W, Cn, 1), **f64) * 2.0 + 3.0
        lo_hi = torch.empty((W, Cn, 2), device=dev, dtype=torch.float64)
        lo_hi[..., 0], lo_hi[..., 1] = x.amin(dim=2), x.amax(dim=2)
        rng = torch.empty((W, Cn, 2), device=dev, dtype=torch.float64)
        cnt = torch.empty((W, Cn, len(cuts), bins + 3), device=dev, dtype=torch.int64)
        st = torch.empty((W, Cn, len(cuts), 2), device=dev, dtype=torch.float64)
        tr = torch.empty((W, Cn, trace[0]), device=dev, dtype=torch.float64)
        torch.cuda.synchronize(dev)
        p = _lib.make_density(W, Cn, nd, nd, cuts, bins, trace, 0, True)
        nbytes = 8.0 * Cn * nd * W
        lines.append("  C = %d columns, %d bins" % (Cn, bins))
        for label, lh, passes in (("automatic range (2 passes)", 0, 2), ("given range (1 pass)", lo_hi.data_ptr(), 1)):
            ms, lo, hi = median_ms(lambda: _lib.chain_density_device(p, x.data_ptr(), lh, rng.data_ptr(), cnt.data_ptr(), st.data_ptr(),
                                                                     tr.data_ptr(), None, True))
            lines.append("    %-28s %8.3f ms   (min %.3f, max %.3f)   %.3f GB read, %.2f TB/s, x %.2f of bytes / 6.3 TB/s"
                         % (label, ms, lo, hi, passes * nbytes / 1e9, passes * nbytes / ms / 1e9, ms / (passes * nbytes / HBM_ACHIEVABLE * 1e3)))
            if Cn == 3 and passes == 2:
                per_byte = ms / (passes * nbytes)
        total = cnt.cpu().numpy()[:, :, -1, :].sum(axis=2)
        lines.append("    counts of the last prefix sum to its cut: %s; results finite: %s"
                     % (bool((total == cuts[-1]).all()), bool(np.isfinite(st.cpu().numpy()).all() and np.isfinite(tr.cpu().numpy()).all())))
        del x, lo_hi, rng, cnt, st, tr
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
              "    %-28s %8.3f ms   (min %.3f, max %.3f)   %.3f GB read, %.2f TB/s" % ("yardstick", ms, lo, hi, mbytes / 1e9, mbytes / ms / 1e9),
              "  time per byte, chain density (C = 3, 64 bins, automatic range) / mixture moments: %.2f" % (per_byte / (ms / mbytes))]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
