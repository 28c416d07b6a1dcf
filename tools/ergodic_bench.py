"""Timing of the ergodic-moment device entry at the production shape, for the record (no threshold).

  python tools/ergodic_bench.py [--W 460] [--nd 250000] [--reps 7] [--out profiles/ergodic_timing.txt]

Prints (and with --out writes): the HIP-event time of hmcg_ergodic_moments_device (median of --reps after a warm-up, with the
range; draws generated on the device) at K = 3 and K = 8, with and without the per-draw columns, round5 on; beside each its
ratio to ONE read of what the kernel reads, 8 W (K^2 + K) nd bytes (the diagonal of A is never read), plus one write of cols,
8 W (2K + 2) nd bytes, where they are kept, at the bandwidth density.hip's range pass reaches in the same session --
hmcg_chain_density_device with the automatic range minus the same call with a given range is that pass.  Then the route a
caller had without this entry, timed by the same tool: A, mu and sig2 copied device -> host and the numpy statements of
hmc.calcergodic over 16 threads (at K = 8 over --host-windows windows, scaled to W)."""
import argparse
import concurrent.futures
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--W", type=int, default=460)
    ap.add_argument("--nd", type=int, default=250000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-windows", type=int, default=46)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from hmc_jl_amd import _lib, hmc
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

    lines = ["Ergodic regime law, durations and long-run moments (hmcg_ergodic_moments_device), one MI355X -- for the record, no threshold.",
             "tools/ergodic_bench.py: W = %d windows, nd = %d draws, round5 on; draws generated on the device (off-diagonal cells uniform" % (W, nd),
             "below 0.02, mu normal about 2 k, sig2 above 0.05); HIP events around the two kernels; median of %d timed calls after one" % a.reps,
             "warm-up call.  One read = 8 W (K^2 + K) nd bytes (the diagonal of A is never read), with cols plus one write of",
             "8 W (2K + 2) nd bytes, at the bandwidth of density.hip's range pass, measured in this session as",
             "hmcg_chain_density_device (64 bins) over a (W, 3, nd) array with the automatic range minus the same call with a given range.", ""]
    # the yardstick: density's range pass
    x = (torch.randn((W, 3, nd), **f64) * 0.3 + 3.0).contiguous()
    lo_hi = torch.empty((W, 3, 2), device=dev, dtype=torch.float64)
    lo_hi[..., 0], lo_hi[..., 1] = x.amin(dim=2), x.amax(dim=2)
    rng = torch.empty((W, 3, 2), device=dev, dtype=torch.float64)
    cnt = torch.empty((W, 3, 1, 64 + 3), device=dev, dtype=torch.int64)
    st = torch.empty((W, 3, 1, 2), device=dev, dtype=torch.float64)
    dp = _lib.make_density(W, 3, nd, nd, None, 64, (0, 1), 0, True)
    torch.cuda.synchronize(dev)
    auto = median_ms(lambda: _lib.chain_density_device(dp, x.data_ptr(), 0, rng.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, None, True))
    given = median_ms(lambda: _lib.chain_density_device(dp, x.data_ptr(), lo_hi.data_ptr(), rng.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, None, True))
    bw = 8.0 * W * 3 * nd / (auto[0] - given[0]) / 1e9                       # TB/s: bytes / ms / 1e9
    lines.append("  density with the automatic range %.3f ms (min %.3f, max %.3f), with a given range %.3f ms (min %.3f, max %.3f):" % (auto + given))
    lines.append("      range pass = one read of %.3f GB in %.3f ms, %.2f TB/s" % (8.0 * W * 3 * nd / 1e9, auto[0] - given[0], bw))
    del x, lo_hi, rng, cnt, st
    for K in (3, 8):
        Cn = _lib.erg_cols(K)
        A = torch.rand((W, K, K, nd), **f64).mul_(0.02)
        mu = torch.randn((W, K, nd), **f64).mul_(0.3).add_(2.0 * torch.arange(K, device=dev, dtype=torch.float64)[None, :, None])
        sig2 = torch.rand((W, K, nd), **f64).add_(0.05)
        out = torch.empty((W, Cn, 2), device=dev, dtype=torch.float64)
        n = torch.empty((W, 2), device=dev, dtype=torch.int64)
        cols = torch.empty((W, Cn, nd), device=dev, dtype=torch.float64)
        p = _lib.make_ergodic(W, K, nd, nd, 0, True)
        torch.cuda.synchronize(dev)
        read, write = 8.0 * W * (K * K + K) * nd, 8.0 * W * Cn * nd
        lines.append("  K = %d: reads %.3f GB, cols %.3f GB" % (K, read / 1e9, write / 1e9))
        for with_cols in (False, True):
            ms, lo, hi = median_ms(lambda: _lib.ergodic_moments_device(p, mu.data_ptr(), sig2.data_ptr(), A.data_ptr(),
                                                                       cols.data_ptr() if with_cols else 0, out.data_ptr(), n.data_ptr(), None, True))
            ideal = (read + (write if with_cols else 0.0)) / bw / 1e9
            lines.append("    %-12s %8.3f ms   (min %.3f, max %.3f)   x %.2f of one read%s (%.3f ms)"
                         % ("with cols" if with_cols else "without cols", ms, lo, hi, ms / ideal, " and one write" if with_cols else "", ideal))
        dev_out, dev_n = out.cpu().numpy(), n.cpu().numpy()
        # the route without this entry: the draws over PCIe, then numpy
        Wh = W if K == 3 else min(W, a.host_windows)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        Ah, mh, sh = A[:Wh].cpu().numpy(), mu[:Wh].cpu().numpy(), sig2[:Wh].cpu().numpy()
        t1 = time.perf_counter()

        def one(w):
            r5 = lambda v: np.rint(v * 1e5) / 1e5
            c = hmc._ergodic_columns(r5(mh[w]).T, r5(sh[w]).T, r5(Ah[w]).reshape(K * K, nd).T)
            return hmc._ergodic_pool(c)
        with concurrent.futures.ThreadPoolExecutor(16) as pool:
            parts = list(pool.map(one, range(Wh)))
        t2 = time.perf_counter()
        same_n = bool(all(np.array_equal(parts[w][1], dev_n[w]) for w in range(Wh)))
        worst = max(float(np.nanmax(np.abs(parts[w][0][:, 0] - dev_out[w, :, 0]) / np.abs(dev_out[w, :, 0]))) for w in range(Wh))
        scale = W / float(Wh)
        lines.append("    without the entry (%d of %d windows%s): copy device -> host %.1f ms + numpy over 16 threads %.1f ms = %.1f ms;"
                     % (Wh, W, "" if Wh == W else ", times scaled by %.0f" % scale, (t1 - t0) * 1e3 * scale, (t2 - t1) * 1e3 * scale, (t2 - t0) * 1e3 * scale))
        lines.append("      the same good counts: %s; pooled means agree to %.1e relative" % (same_n, worst))
        del A, mu, sig2, cols, out, n, Ah, mh, sh
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
