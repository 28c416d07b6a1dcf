"""Timing of the exact-quantile device entry at the production shape, for the record (no threshold).

  python tools/chain_quantiles_bench.py [--W 460] [--nd 250000] [--reps 7] [--out profiles/chain_quantiles_timing.txt]

Prints (and with --out writes): the HIP-event time of hmcg_chain_quantiles_device (median of --reps after a warm-up, with the
spread; draws generated on the device) at C = 3 and 9 columns, Q = 3 (0.05, 0.5, 0.95) and Q = 16 probabilities, round5 on and
off; beside each its ratio to ONE read of the draws, 8 W C nd bytes, at the bandwidth density.hip's range pass reaches in the
same session -- hmcg_chain_density_device with the automatic range minus the same call with a given range is that pass.  The
selection reads a column at most 8 times, so 8 is the design's ceiling of that ratio.  Then the route a caller had without this
entry, timed by the same tool: the same input copied device -> host and np.quantile over 16 threads.  For C = 3, Q = 3 one
host-entry call (call_ms: upload in groups of whole columns, kernels, results)."""
import argparse
import concurrent.futures
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROBS3 = (0.05, 0.5, 0.95)
PROBS16 = tuple(float(p) for p in np.linspace(0.025, 0.975, 16))


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

    lines = ["Exact quantiles by selection (hmcg_chain_quantiles_device), one MI355X -- for the record, no threshold.",
             "tools/chain_quantiles_bench.py: W = %d windows, nd = %d draws; draws generated on the device (a normal about a centre per" % (W, nd),
             "column; every third column a pi_end-like one, 90 %% of its draws exactly 1); HIP events around the kernel; median of %d" % a.reps,
             "timed calls after one warm-up call.  One read = 8 W C nd bytes at the bandwidth of density.hip's range pass, measured in",
             "this session as hmcg_chain_density_device (64 bins) with the automatic range minus the same call with a given range.", ""]
    host_route = None
    for Cn in (3, 9):
        x = torch.randn((W, Cn, nd), **f64) * 0.3 + torch.randn((W, Cn, 1), **f64) * 2.0 + 3.0
        ties = torch.rand((W, Cn // 3, nd), **f64) < 0.9
        x[:, 2::3, :] = torch.where(ties, torch.ones((), device=dev, dtype=torch.float64), torch.rand((W, Cn // 3, nd), **f64))
        del ties
        x = x.contiguous()
        nbytes = 8.0 * W * Cn * nd
        # the yardstick: density's range pass
        lo_hi = torch.empty((W, Cn, 2), device=dev, dtype=torch.float64)
        lo_hi[..., 0], lo_hi[..., 1] = x.amin(dim=2), x.amax(dim=2)
        rng = torch.empty((W, Cn, 2), device=dev, dtype=torch.float64)
        cnt = torch.empty((W, Cn, 1, 64 + 3), device=dev, dtype=torch.int64)
        st = torch.empty((W, Cn, 1, 2), device=dev, dtype=torch.float64)
        dp = _lib.make_density(W, Cn, nd, nd, None, 64, (0, 1), 0, True)
        torch.cuda.synchronize(dev)
        auto = median_ms(lambda: _lib.chain_density_device(dp, x.data_ptr(), 0, rng.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, None, True))
        given = median_ms(lambda: _lib.chain_density_device(dp, x.data_ptr(), lo_hi.data_ptr(), rng.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, None, True))
        one_read = auto[0] - given[0]
        lines.append("  C = %d columns: density with the automatic range %.3f ms (min %.3f, max %.3f), with a given range %.3f ms (min %.3f, max %.3f):"
                     % ((Cn,) + auto + given))
        lines.append("      range pass = one read of %.3f GB in %.3f ms, %.2f TB/s" % (nbytes / 1e9, one_read, nbytes / one_read / 1e9))
        del lo_hi, rng, cnt, st
        for probs in (PROBS3, PROBS16):
            for r5 in (True, False):
                q = torch.empty((W, Cn, len(probs), _lib.ORD_STRIDE), device=dev, dtype=torch.float64)
                n = torch.empty((W, Cn, 2), device=dev, dtype=torch.int64)
                qp = _lib.make_quantiles(W, Cn, nd, nd, probs, 0, r5)
                torch.cuda.synchronize(dev)
                ms, lo, hi = median_ms(lambda: _lib.chain_quantiles_device(qp, x.data_ptr(), q.data_ptr(), n.data_ptr(), None, True))
                lines.append("    Q = %2d, round5 %-3s  %8.3f ms   (min %.3f, max %.3f)   x %.2f of one read (ceiling 8)"
                             % (len(probs), "on" if r5 else "off", ms, lo, hi, ms / one_read))
                if Cn == 3 and probs is PROBS3 and not r5:
                    dev_q = _lib.unpack_chain_quantiles(q.cpu().numpy(), n.cpu().numpy())
                del q, n
        if Cn == 3:
            # the route without this entry: every draw over PCIe, then the host sorts
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            xh = x.cpu().numpy()
            t1 = time.perf_counter()
            with concurrent.futures.ThreadPoolExecutor(16) as pool:
                parts = list(pool.map(lambda w: np.quantile(xh[w], PROBS3, axis=1), range(W)))
            t2 = time.perf_counter()
            want = np.stack(parts).transpose(0, 2, 1)                      # (W, C, Q)
            agree = bool((np.abs(dev_q["value"] - want) <= 2.0 ** -51 * (np.abs(dev_q["lo"]) + np.abs(dev_q["hi"]))).all())
            tm = _lib.Timing()
            host = _lib.chain_quantiles(xh, PROBS3, round5=False, timing=tm)
            same = all(np.array_equal(host[k], dev_q[k], equal_nan=True) for k in dev_q)
            host_route = ["", "  The same quantiles (C = 3, Q = 3, round5 off) without the device entry:",
                          "    copy device -> host %.1f ms + np.quantile over 16 threads %.1f ms = %.1f ms; agrees with the device to 2^-51 (|lo| + |hi|): %s"
                          % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3, agree),
                          "    hmcg_chain_quantiles (host entry, %d uploads of whole columns): call_ms %.1f, kernel_ms %.3f; the same bits as the device entry: %s"
                          % (tm.launches, tm.call_ms, tm.kernel_ms, same)]
            del xh, host
        del x
    lines += host_route
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
