"""What one sweep reports, recomputed from the call's own outputs -- no oracle, no random numbers.  A plain module for
tests/test_sweep_identities.py (the oracle, no GPU) and tests/test_gpu_sweep_identities.py (every smoothing-capable kernel form);
importing it needs neither torch nor a GPU.

With nrun = 1 and n_samples = 1 a call returns everything the reference's formulas need for its one kept sweep, all in sorted
labels: the draw's mu, sig2 and A; pi_filter_mean = that sweep's filtered probabilities pif; pi_smooth_mean = pi_smooth_draws =
its smoothed probabilities pib; pi_end, fcast, and sigvals (with save_range = sig_range: Yfake over the signal range).
residuals() evaluates in numpy.longdouble, each identity from t = 1 on from the RETURNED pif[t-1] (rho is not returned and
not needed):
  filter step  (forwardupdate_P!, src/Hmc.jl:371-440)  P_t[r,s] = pif[t-1,r] A[r,s] N(Yfake[t]; mu[s], sd[s] (1+kappa if t is a
               signal step else 1)) / total;  sum_r P_t[r,s] against pif[t,s]
  smoother     (backwardupdate_P!, :442-457)  pib[T-1] = pif[T-1], pib[t,r] = sum_s P_{t+1}[r,s] pib[t+1,s] / pif[t+1,s], against
               the returned pib at every step
  reported row (:900)  pi_end against the recomputed pib[end_pos] (pib[T-1] without end_pos)
  forecasts    (forecast :658-667, forecastsignal :670-681)  pif[T-1]' A^h mu by h products; slots of blend_mask
               a Yfake[T-1] + (1-a) pif[T-1]' mu, a = tau / (1 + tau), tau = 1 / sigma_signal; relative to 1 + |ref|

CASES is the table both test modules run: the smallest shapes that still reach each smoothing-capable kernel form (the
register-resident SM rows in every flavour, the SIG + SM rows, the four smoothing forms of the LDS-resident kernel), among them
what no other GPU test passes: end_pos together with a smoothing output, where the device builds pi_end by a backward vector
product of its own beside the full smoother.  tests/test_variant_coverage.py holds the table to the parsed variant tables."""
import numpy as np

from hmc_jl_amd import synth
from kernel_tables import NT, STREAM_T, ladder_ceiling

LD = np.longdouble
IDENTITIES = ("filter", "smoother", "row", "forecast")
KAPPA, ALPHA_SIG = 0.6, 2.0                      # the signal paths' kappa and alpha = nu
MAXTAIL = 256                                    # HMCG_MAXTAIL (tests/test_sweep_identities.py holds it to _lib's)
TAIL_HORIZONS, TAIL_BLEND = (0, 12), 1           # slot 0 is the blend (h == sigLen), slot 1 is h = sigLen + 12


def normpdf_ld(y, mu, sd):
    z = (y - mu) / sd
    return np.exp(LD(-0.5) * z * z) / (sd * np.sqrt(LD(2) * LD(4) * np.arctan(LD(1))))


def residuals(mu, sig2, A, pif, pib, pi_end, fcast, yfake, horizons, sig=None, kappa=0.0, end_pos=None, blend_mask=0,
              sigma_signal=0.0, lag=1):
    """The four residuals of one window's one kept sweep (see the module docstring), in numpy.longdouble.
    mu, sig2 (K,), A (K, K) with A[r, s] = P(r -> s), pif, pib (T, K), pi_end (K,): sorted labels.  fcast (H,): the forecast
    values (not the error columns) of `horizons`.  yfake (T,): the data the sweep ran on.  sig: the half-open signal range
    (None: empty).  end_pos: None = the last step.  lag: the filter step's predecessor row is pif[t - lag]; 1 is the reference's
    (0 exists for the test that shows the checker can fail).
    Returns {"filter", "smoother", "row", "forecast": the largest residual of that identity; "min_pif"; "left_out": the share of
    the T - 1 steps that could not be checked (a zero filtered probability or emission total: 0/0); "at": {identity: where its
    largest residual sits -- (t, state) or the horizon slot}}."""
    mu, sig2, A = np.asarray(mu, LD), np.asarray(sig2, LD), np.asarray(A, LD)
    pif, pib, y = np.asarray(pif, LD), np.asarray(pib, LD), np.asarray(yfake, LD)
    T, K = pif.shape
    assert pib.shape == (T, K) and y.shape == (T,) and A.shape == (K, K) and T >= 2
    scale = np.ones((T, 1), LD)
    if sig is not None and sig[0] < sig[1]:
        scale[int(sig[0]):int(sig[1])] = LD(1) + LD(kappa)
    f = normpdf_ld(y[:, None], mu[None, :], np.sqrt(sig2)[None, :] * scale)              # (T, K)
    # ---- filter step, t = 1 .. T-1 ----
    num = (pif[1 - lag:T - lag] @ A) * f[1:]                                             # sum_r pif[t-1,r] A[r,s] f_t[s]
    total = num.sum(axis=1)
    ok = (total > 0) & (pif[1:] > 0).all(axis=1) & (pif[:-1] > 0).all(axis=1)
    safe = np.where(ok, total, LD(1))
    dfl = np.where(ok[:, None], np.abs(num / safe[:, None] - pif[1:]), LD(0))
    i, s = np.unravel_index(np.argmax(dfl), dfl.shape)
    at = {"filter": (int(i) + 1, int(s))}
    # ---- smoother: pib[t,r] = pif[t,r] sum_s (A[r,s] f_{t+1}[s] / total_{t+1}) pib[t+1,s] / pif[t+1,s] ----
    G = A[None, :, :] * (f[1:] / safe[:, None])[:, None, :]                              # (T-1, K, K)
    ref = np.empty((T, K), LD)
    ref[T - 1] = pif[T - 1]
    for t in range(T - 2, -1, -1):
        ref[t] = pif[t] * (G[t] @ (ref[t + 1] / pif[t + 1])) if ok[t] else pib[t]       # (an unchecked step restarts from the returned row)
    dsm = np.abs(ref - pib)
    dsm[:-1][~ok] = 0
    at["smoother"] = tuple(int(i) for i in np.unravel_index(np.argmax(dsm), dsm.shape))
    # ---- reported row ----
    rep = T - 1 if end_pos is None else int(end_pos)
    assert 0 <= rep <= T - 1
    drow = np.abs(np.asarray(pi_end, LD) - ref[rep])
    at["row"] = (rep, int(np.argmax(drow)))
    # ---- forecasts ----
    dfc = np.zeros(len(horizons), LD)
    for k, h in enumerate(horizons):
        if (blend_mask >> k) & 1:
            tau = LD(1) / LD(sigma_signal)
            a = tau / (LD(1) + tau)
            want = a * y[T - 1] + (LD(1) - a) * (pif[T - 1] @ mu)
        else:
            v = pif[T - 1]
            for _ in range(int(h)):
                v = v @ A
            want = v @ mu
        dfc[k] = abs(LD(fcast[k]) - want) / (LD(1) + abs(want))
    at["forecast"] = int(np.argmax(dfc)) if len(horizons) else None
    return dict(filter=float(dfl.max()), smoother=float(dsm.max()), row=float(drow.max()), forecast=float(dfc.max()) if len(horizons) else 0.0,
                min_pif=float(pif.min()), left_out=float((~ok).sum()) / (T - 1), at=at)


# ---- the case table ----
def _case(id, kernel, path, K, lens, L=None, flavour=None, sig_len=None, tail=None, ssig=None):
    """kernel: register | lds | stream (what the production dispatch must pick; register: row (K, L), HMCG_FLAVOUR = flavour,
    None: the table's own choice).  path: smooth (base path) | sig+smooth (sigLen = 0) | tail+smooth (signals past the end date).
    sig_len[w]: signal steps at the end of window w (None: all of it).  tail[w]: sigLen, end_pos = T - 1 - sigLen."""
    return dict(id=id, kernel=kernel, path=path, K=K, lens=list(lens), L=L, flavour=flavour, sig_len=sig_len, tail=tail, ssig=ssig)


def _class_lens(L):
    """Three ragged lengths inside the steps-per-thread class of L (256 (L/2) < T <= 256 L: one launch, no length buckets); the
    longest is odd and just under the row's capacity, at L = 4 one lies in 513..768 and two in 769..1024."""
    return {1: [255, 130, 66], 2: [511, 450, 258], 4: [1023, 771, 600], 8: [2047, 1500, 1026]}[L]


def _tail_case(id, kernel, K, top, lo, L, top_tail, ssig=(0.4, 1.3, 0.4)):
    """Signals past the end date with smoothing outputs: the longest window (sigLen = top_tail), one whose end_pos is the last
    step of a wave's share of the window (64 L j - 1) and one whose end_pos is the first step of the next wave's (64 L j): the
    backward product over the tail crosses the lane and wave boundary there.  lo: the shortest length of the kernel's class.
    The three windows carry sigLen 1, 12 and HMCG_MAXTAIL between them wherever the class is long enough for the last."""
    rest = [n for n in (1, 12, MAXTAIL) if n != top_tail] if top_tail in (1, 12, MAXTAIL) else [12, 1]
    span = 64 * L
    wins, tails = [top], [top_tail]
    for edge, n in zip((-1, 0), sorted(rest, reverse=True)):
        j = 1
        while span * j + edge + 1 + n < lo:
            j += 1
        T = span * j + edge + 1 + n                       # end_pos = span j + edge
        assert lo <= T <= top and n <= T - 1, (id, T, n)
        wins.append(T)
        tails.append(n)
    return _case(id, kernel, "tail+smooth", K, wins, L=L, tail=tails, ssig=list(ssig))


def _big_top(K, sig):
    """One window past the register-resident ladder of the path (ladder_ceiling, from the parsed tables); no multiple of 256."""
    return max(ladder_ceiling(K, sig, True), 2 * NT) + 45


def _build_cases():
    cases = []
    # base path, register-resident SM rows: every flavour at L = 1 and L = 4, one flavour at L = 2, (3, 8) on p1
    for K in (2, 3, 4):
        for L in (1, 4):
            for fl in ("h", "p1", "p2"):
                cases.append(_case("reg-sm-K%d-L%d-%s" % (K, L, fl), "register", "smooth", K, _class_lens(L), L=L, flavour=fl))
        cases.append(_case("reg-sm-K%d-L2-%s" % (K, ("h", "p1", "p2")[K - 2]), "register", "smooth", K, _class_lens(2), L=2,
                           flavour=("h", "p1", "p2")[K - 2]))
    cases.append(_case("reg-sm-K3-L8-p1", "register", "smooth", 3, _class_lens(8), L=8, flavour="p1"))
    # base path, LDS-resident smoothing form g_big_010 and its streaming form g_big_011
    cases.append(_case("lds-sm-K3", "lds", "smooth", 3, [_big_top(3, False), 300, 65]))
    cases.append(_case("lds-sm-K5", "lds", "smooth", 5, [600, 257, 65]))
    cases.append(_case("lds-sm-K8", "lds", "smooth", 8, [601, 300, 64]))
    cases.append(_case("stream-sm-K3", "stream", "smooth", 3, [STREAM_T, 1000]))
    # signal path, sigLen = 0
    cases.append(_case("reg-sigsm-K3-L2", "register", "sig+smooth", 3, [511, 400, 300], L=2, sig_len=[40, 40, 1], ssig=[0.5, 0.2, 0.8]))
    cases.append(_case("reg-sigsm-K3-allsignal", "register", "sig+smooth", 3, [120, 200], L=1, sig_len=[None, 12], ssig=[0.5, 0.3]))
    cases.append(_case("lds-sigsm-K6", "lds", "sig+smooth", 6, [300, 297, 150], sig_len=[40, 1, None], ssig=[0.5, 0.8, 0.2]))
    # signals past the end date with smoothing outputs
    cases.append(_tail_case("reg-tailsm-K2-L1", "register", 2, 256, 30, 1, 100))
    cases.append(_tail_case("reg-tailsm-K3-L4", "register", 3, 1023, 513, 4, MAXTAIL))
    cases.append(_tail_case("reg-tailsm-K3-L8", "register", 3, 2047, 1025, 8, 12, ssig=(1.3, 0.4, 1.3)))
    cases.append(_tail_case("reg-tailsm-K4-L4", "register", 4, 1024, 513, 4, 1, ssig=(1.3, 0.4, 0.4)))
    for K, top in ((3, _big_top(3, True)), (5, 600), (8, 515)):
        cases.append(_tail_case("lds-tailsm-K%d" % K, "lds", K, top, 30, (top + NT - 1) // NT, MAXTAIL if K != 5 else 12,
                                ssig=(0.4, 1.3, 1.3) if K != 5 else (1.3, 0.4, 0.4)))
    cases.append(_tail_case("stream-tailsm-K3", "stream", 3, STREAM_T, 30, (STREAM_T + NT - 1) // NT, MAXTAIL))
    for i, c in enumerate(cases):
        c["burnin"] = i % 4                               # the kernels pick buffers by sweep parity
        c["window_ids"] = [(5 + 3 * i + 7 * w) % 97 for w in range(len(c["lens"]))]
    return cases


CASES = _build_cases()
CASE_IDS = [c["id"] for c in CASES]
# the further tail-with-smoothing call per form against the oracle alone (n_samples = 3, nrun = 4: sample parity selects the
# staged last observation), and the two that also go through the device entry
MULTI_SAMPLE = ("reg-tailsm-K3-L4", "lds-tailsm-K5", "stream-tailsm-K3")
DEVICE_ENTRY = ("reg-tailsm-K3-L8", "lds-tailsm-K8")


def case_by_id(id):
    return CASES[CASE_IDS.index(id)]


def call_of(c, n_samples=1, nrun=1):
    """(args, kw) of the case's call for _lib.estimate_batch_host / device_entry.estimate_batch_device_np."""
    K, lens = c["K"], c["lens"]
    W = len(lens)
    Y, Tw, fut = synth.generate_panel(W, max(lens), K, ragged=lens)
    kw = dict(want_state=True, want_smooth=True, want_filter_mean=True, want_smooth_draws=True, window_ids=np.array(c["window_ids"]))
    horizons, yreal = (1, 12), fut[:, [0, 11]]
    if c["path"] != "smooth":
        n = np.array([T if m is None else m for T, m in zip(Tw, c["tail"] or c["sig_len"])])
        sig = np.stack([Tw - n, Tw], axis=1).astype(np.int32)
        kw.update(sig_range=sig, save_range=sig, sigma_signal=np.array(c["ssig"], dtype=np.float64), kappa=KAPPA, n_samples=n_samples,
                  alpha=ALPHA_SIG, nu=ALPHA_SIG)
    if c["path"] == "tail+smooth":
        horizons = TAIL_HORIZONS
        kw.update(end_pos=(Tw - 1 - np.array(c["tail"])).astype(np.int32), blend_mask=TAIL_BLEND)
    return (Y, Tw, K, c["burnin"], nrun, horizons, yreal), kw


def oracle_window(oracle, args, kw, w, n_samples=1):
    """The oracle's run of window w of a case's call."""
    Y, Tw, K, burnin, nrun, horizons, yreal = args
    T = int(Tw[w])
    more = {}
    if "sig_range" in kw:
        more = dict(sig=tuple(int(v) for v in kw["sig_range"][w]), save=tuple(int(v) for v in kw["save_range"][w]), kappa=kw["kappa"],
                    alpha=kw["alpha"], nu=kw["nu"], sigma_signal=float(kw["sigma_signal"][w]))
    if "end_pos" in kw:
        more.update(end_pos=int(kw["end_pos"][w]), blend_mask=kw["blend_mask"])
    return oracle.estimate_signals(Y[w, :T], K, burnin, nrun, n_samples, horizons=horizons, yreal=yreal[w], window_id=int(kw["window_ids"][w]),
                                   want_smooth=True, want_filter_mean=True, **more)


def _yfake(args, kw, w, sigvals):
    Y, Tw = args[0], args[1]
    y = np.array(Y[w, :int(Tw[w])])
    if "sig_range" in kw:
        b, e = (int(v) for v in kw["sig_range"][w])
        y[b:e] = sigvals[:e - b]
    return y


def _window_kw(args, kw, w):
    out = dict(horizons=args[5])
    if "sig_range" in kw:
        out.update(sig=tuple(int(v) for v in kw["sig_range"][w]), kappa=kw["kappa"], sigma_signal=float(kw["sigma_signal"][w]))
    if "end_pos" in kw:
        out.update(end_pos=int(kw["end_pos"][w]), blend_mask=kw["blend_mask"])
    return out


def oracle_inputs(args, kw, w, o):
    """residuals()'s arguments from the oracle's one-draw run of window w: (positional, keywords)."""
    assert o["mu"].shape[0] == 1
    yf = _yfake(args, kw, w, o["sigvals"][0] if "sig_range" in kw else None)
    return (o["mu"][0], o["sig2"][0], o["A"][0], o["pi_filter_mean"], o["pi_smooth"][0], o["pi_end"][0], o["fcast"][0, 0::2], yf), _window_kw(args, kw, w)


def library_inputs(args, kw, w, g):
    """The same from a result of the library's host or device entry (C-ABI layouts, one kept draw)."""
    T = int(args[1][w])
    assert g["mu"].shape[2] == 1
    yf = _yfake(args, kw, w, g["sigvals"][w, 0] if "sig_range" in kw else None)
    return (g["mu"][w, :, 0], g["sig2"][w, :, 0], g["A"][w, :, :, 0].T, g["pi_filter_mean"][w, :T], g["pi_smooth_mean"][w, :T], g["pi_end"][w, :, 0],
            g["fcast"][w, 0::2, 0], yf), _window_kw(args, kw, w)


def describe(r):
    """One line per window for an assertion message: which identity, how much, where."""
    return ", ".join("%s %.2e at %s" % (k, r[k], r["at"][k]) for k in IDENTITIES) + ", min pif %.1e, left out %.3g" % (r["min_pif"], r["left_out"])


_ORACLE_RUNS = {}


def oracle_runs(oracle, c):
    """(args, kw, [the oracle's one-draw run of every window]) of a case: computed once, shared by the tests, never changed."""
    if c["id"] not in _ORACLE_RUNS:
        args, kw = call_of(c)
        _ORACLE_RUNS[c["id"]] = (args, kw, [oracle_window(oracle, args, kw, w) for w in range(len(c["lens"]))])
    return _ORACLE_RUNS[c["id"]]
