"""Timing of the predictive-score device entry at the production shape, for the record (no threshold).

  python tools/score_bench.py [--W 460] [--nd 250000] [--reps 7] [--K 3 8] [--exact-nd 20000] [--out profiles/score_timing.txt]

For K = 3 and K = 8, horizons (0, 12), default thinning: the HIP-event time of hmcg_predictive_scores_device (median of --reps
after a warm-up; draws generated on the device) and, as the yardstick, hmcg_predictive_cdf_device in the same session on the
same draws and horizons with G = 81 grid points.  The score entry is counted in pair terms -- the a(m, S2) it evaluates: per
row of tiles its components times the components up to the end of its diagonal tile -- the CDF entry in Phi evaluations; the
ratio of the two rates is written down.  Then one exact window (stride 1) of --exact-nd draws at K = 3.  The text goes to --out
as well as to the terminal."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TP = 256


def pair_terms(N):
    """a(m, S2) evaluations of one window of N components: tiles on and below the diagonal, whole where they are whole."""
    nT = -(-N // TP)
    return sum(min(TP, N - r * TP) * min((r + 1) * TP, N) for r in range(nT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--W", type=int, default=460)
    ap.add_argument("--nd", type=int, default=250000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--G", type=int, default=81)
    ap.add_argument("--K", type=int, nargs="+", default=[3, 8])
    ap.add_argument("--exact-nd", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "score_timing.txt"))
    a = ap.parse_args()
    import torch
    from hmc_jl_amd import _lib
    _lib.load()
    dev = torch.device("cuda", 0)
    W, nd, G = a.W, a.nd, a.G
    hz = (0, 12)
    stride, n_u = _lib.score_thinning(nd, 0)
    lines = ["Predictive scores (hmcg_predictive_scores_device), production shape, one MI355X -- for the record, no threshold.",
             "tools/score_bench.py: W = %d windows, nd = %d draws, horizons %s, default thinning (stride %d, %d used draws), round5 on;" % (W, nd, hz, stride, n_u),
             "draws generated on the device; HIP events around the 3 kernels of a call; median of %d timed calls after one warm-up call." % a.reps,
             "Yardstick: hmcg_predictive_cdf_device in the same session on the same draws and horizons, G = %d." % G,
             ""]

    def median_ms(call):
        times = []
        for rep in range(a.reps + 1):
            tm = call()
            if rep:
                times.append(tm.kernel_ms)
        return statistics.median(times), min(times), max(times)

    def draws(Wn, K, n, g):
        mu = torch.randn((Wn, K, n), generator=g, device=dev, dtype=torch.float64) * 3.0 + 2.0
        sig2 = torch.rand((Wn, K, n), generator=g, device=dev, dtype=torch.float64) * 4.0 + 0.05
        pi = torch.rand((Wn, K, n), generator=g, device=dev, dtype=torch.float64) + 0.01
        pi /= pi.sum(dim=1, keepdim=True)
        A = torch.rand((Wn, K, K, n), generator=g, device=dev, dtype=torch.float64) + 0.01
        A /= A.sum(dim=1, keepdim=True)             # A[w, j, i, d]: row i sums to 1 over j
        return mu, sig2, pi, A

    def score_call(Wn, K, n, st, mu, sig2, pi, A):
        y = torch.full((len(hz), Wn), 2.5, device=dev, dtype=torch.float64)
        out = torch.empty((Wn, len(hz), _lib.SCORE_STRIDE), device=dev, dtype=torch.float64)
        torch.cuda.synchronize(dev)
        sc = _lib.make_score(Wn, K, n, n, hz, st, 0, True)
        ms = median_ms(lambda: _lib.predictive_scores_device(sc, mu.data_ptr(), sig2.data_ptr(), pi.data_ptr(), A.data_ptr(), y.data_ptr(),
                                                             out.data_ptr(), None, True))
        return ms, out.cpu().numpy()

    grid = torch.from_numpy(np.linspace(-5.0, 15.0, G)).to(dev)
    for K in a.K:
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        mu, sig2, pi, A = draws(W, K, nd, g)
        (s_ms, s_lo, s_hi), out = score_call(W, K, nd, 0, mu, sig2, pi, A)
        cdf = torch.empty((W, len(hz), G), device=dev, dtype=torch.float64)
        pred = _lib.make_predictive(W, K, nd, nd, G, hz, 0, True)
        c_ms, c_lo, c_hi = median_ms(lambda: _lib.predictive_cdf_device(pred, mu.data_ptr(), sig2.data_ptr(), pi.data_ptr(), A.data_ptr(),
                                                                        grid.data_ptr(), cdf.data_ptr(), None, True))
        terms = float(W) * pair_terms(n_u * K)
        c_phi = float(W) * nd * K * len(hz) * G
        s_rate, c_rate = terms / (s_ms * 1e-3), c_phi / (c_ms * 1e-3)
        lines += ["K = %d" % K,
                  "  score entry      %9.2f ms   (min %.2f, max %.2f; %.3e pair terms, %.3e pair terms/s; mean crps %.4f)"
                  % (s_ms, s_lo, s_hi, terms, s_rate, float(out[..., 0].mean())),
                  "  CDF entry        %9.2f ms   (min %.2f, max %.2f; %.3e Phi, %.3e Phi/s)" % (c_ms, c_lo, c_hi, c_phi, c_rate),
                  "  pair terms/s over Phi/s   %.3f" % (s_rate / c_rate),
                  ""]
        print("\n".join(lines[-5:]), flush=True)
        del mu, sig2, pi, A, cdf
        torch.cuda.empty_cache()
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    K, n = 3, a.exact_nd
    mu, sig2, pi, A = draws(1, K, n, g)
    (s_ms, s_lo, s_hi), out = score_call(1, K, n, 1, mu, sig2, pi, A)
    terms = float(pair_terms(n * K))
    lines += ["exact route: one window, stride 1, nd = %d, K = %d (N = %d components, %d blocks)" % (n, K, n * K, (-(-n * K // TP) + 1) // 2),
              "  score entry      %9.2f ms   (min %.2f, max %.2f; %.3e pair terms, %.3e pair terms/s)" % (s_ms, s_lo, s_hi, terms, terms / (s_ms * 1e-3)),
              ""]
    print("\n".join(lines[-3:]), flush=True)
    text = "\n".join(lines)
    with open(a.out, "w") as fh:
        fh.write(text)
    print("written to %s" % a.out)


if __name__ == "__main__":
    main()
