"""Timing of the predictive-CDF device entry at the production shape, for the record (no threshold).

  python tools/predictive_bench.py [--W 460] [--nd 250000] [--K 3] [--G 81] [--reps 7] [--no-host]

Prints: the HIP-event time of hmcg_predictive_cdf_device (median of --reps after a warm-up; draws generated on the device),
the time of the numpy file-route formula (hmc._cdfs_from_cells) on ONE window of the same shape, and the instruction-issue
floor of the accumulation loop: the fp64 instructions per Phi counted in the kernel's own ISA (csrc/obj/predictive-*.s, K = 3:
226 per draw = 75.3 per Phi, one branch-free block) x the Phi count / (1024 SIMDs x 16 fp64 lanes per cycle x 2.4 GHz; the
fp64 pipe takes 4 cycles per wave-instruction, profiles/r04/ubench_op_issue.txt)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_PER_DRAW = {3: 226}          # fp64 VALU instructions of one trip of the K = 3 accumulation loop (.LBB of ds_read2_b64 + 3 erfc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--W", type=int, default=460)
    ap.add_argument("--nd", type=int, default=250000)
    ap.add_argument("--K", type=int, default=3)
    ap.add_argument("--G", type=int, default=81)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import torch
    from hmc_jl_amd import _lib, hmc
    _lib.load()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    W, K, nd, G = a.W, a.K, a.nd, a.G
    mu = torch.randn((W, K, nd), generator=g, device=dev, dtype=torch.float64) * 3.0 + 2.0
    sig2 = torch.rand((W, K, nd), generator=g, device=dev, dtype=torch.float64) * 4.0 + 0.05
    pi = torch.rand((W, K, nd), generator=g, device=dev, dtype=torch.float64) + 0.01
    pi /= pi.sum(dim=1, keepdim=True)
    ys = np.linspace(-5.0, 15.0, G)
    grid = torch.from_numpy(ys).to(dev)
    out = torch.empty((W, 1, G), device=dev, dtype=torch.float64)
    torch.cuda.synchronize(dev)
    pred = _lib.make_predictive(W, K, nd, nd, G, (0,), 0, True)
    times = []
    for rep in range(a.reps + 1):
        tm = _lib.predictive_cdf_device(pred, mu.data_ptr(), sig2.data_ptr(), pi.data_ptr(), 0, grid.data_ptr(), out.data_ptr(), None, True)
        if rep:
            times.append(tm.kernel_ms)
    dev_ms = statistics.median(times)
    nphi = float(W) * nd * G * K
    print("device entry  W=%d nd=%d K=%d G=%d: median %.2f ms of %d (min %.2f, max %.2f) = %.2f ps per Phi"
          % (W, nd, K, G, dev_ms, len(times), min(times), max(times), dev_ms * 1e9 / nphi))
    if K in FP64_PER_DRAW:
        per_phi = FP64_PER_DRAW[K] / K
        floor_ms = per_phi * nphi / (1024 * 16 * 2.4e9) * 1e3
        waves = -(-G // 64) * 64 / G
        print("issue floor   %.1f fp64 instructions per Phi: %.2f ms (device / floor = %.2f); with %d of %d lanes of the item waves "
              "live: %.2f ms (device / that = %.2f)" % (per_phi, floor_ms, dev_ms / floor_ms, G, -(-G // 64) * 64,
                                                        floor_ms * waves, dev_ms / (floor_ms * waves)))
    if not a.no_host:
        c = lambda t: np.round(t[0].T.cpu().numpy(), 5)
        means, vars_, pis = c(mu), c(sig2), c(pi)
        t0 = time.perf_counter()
        bar = hmc._cdfs_from_cells(means, vars_, pis, None, ys, (0,))
        host_ms = (time.perf_counter() - t0) * 1e3
        err = float(np.abs(bar[0] - out[0, 0].cpu().numpy()).max())
        print("numpy formula ONE window nd=%d: %.0f ms; x %d windows = %.0f s; device (all windows) / numpy (all windows) = 1 / %.0f; "
              "max |diff| on that window %.2e" % (nd, host_ms, W, host_ms * W / 1e3, host_ms * W / dev_ms, err))


if __name__ == "__main__":
    main()
