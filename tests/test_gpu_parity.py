"""GPU parity tests proper: the HIP path, called through the C ABI, against the oracle on the
same seeded inputs (the bar and the comparison: tests/oracle_parity.py)."""
import numpy as np
import pytest

from hmc_jl_amd import _lib, synth
from oracle_parity import (FLOAT_KEYS, TOL, assert_same, assert_window_matches_oracle, check_against_oracle, check_signals_against_oracle,
                           check_tail_signals_against_oracle, check_teacher_forced_against_oracle, close)

pytestmark = pytest.mark.gpu
DRAWS = ("mu", "sig2", "A", "pi_end", "fcast", "summary")


def test_cfg1_plumbing_case(hmclib, oracle):
    """BASELINE configs[0]: 3-state, T=200, 1 window, 100 draws."""
    Y, Tw, fut = synth.generate_panel(1, 200, 3)
    check_against_oracle(oracle, Y, Tw, 3, 0, 100, (12,), fut[:, 11:12])


@pytest.mark.parametrize("K", [2, 3, 4])
def test_ragged_windows_all_chunkings(hmclib, oracle, K):
    """Ragged panel crossing every steps-per-thread variant boundary (L=1,2,4,8 at 256 threads)
    and the wave boundaries (63/64/65, 255/256/257)."""
    lens = [2, 3, 5, 63, 64, 65, 200, 255, 256, 257, 511, 513, 1000, 1024, 1025, 2047]
    Y, Tw, fut = synth.generate_panel(len(lens), max(lens), K, ragged=lens)
    for sub in ([0, 1, 2, 3, 4, 5, 6, 7, 8], [9, 10], [11, 12, 13], [14, 15]):
        idx = np.array(sub)
        ld = int(Tw[idx].max())
        check_against_oracle(oracle, np.ascontiguousarray(Y[idx, :ld]), Tw[idx], K, 3, 12, (12,), fut[idx, 11:12],
                             window_ids=idx)


@pytest.mark.parametrize("K", [5, 6, 7, 8])
def test_large_k_kernel(hmclib, oracle, K):
    """The large-K variant (LDS-resident window, fused filter-replay/state-map construction)."""
    lens = [2, 64, 65, 300, 700, 1000]
    Y, Tw, fut = synth.generate_panel(len(lens), max(lens), K, ragged=lens)
    check_against_oracle(oracle, Y, Tw, K, 3, 10, (1, 12), fut[:, [0, 11]])


def test_long_window_small_k_uses_lds_resident_kernel(hmclib, oracle):
    """K=3 with T beyond the register-resident variants (4096): served by the LDS-resident kernel."""
    Y, Tw, fut = synth.generate_panel(2, 5000, 3)
    g = check_against_oracle(oracle, Y, Tw, 3, 2, 6, (12,), fut[:, 11:12])
    assert g["steps_per_thread"] == 20 and g["lds_bytes"] > 100000


def test_cfg4_shape_8_states_T5000(hmclib, oracle):
    """BASELINE configs[3] shape (8-state, T=5000) on a few windows, fewer draws; full-size properties."""
    K, T, W = 8, 5000, 3
    Y, Tw, fut = synth.generate_panel(W, T, K)
    g = check_against_oracle(oracle, Y, Tw, K, 2, 6, (12,), fut[:, 11:12])
    A = np.transpose(g["A"], (0, 3, 2, 1))
    assert np.max(np.abs(A.sum(axis=3) - 1)) < 1e-12 and (np.diff(np.transpose(g["mu"], (0, 2, 1)), axis=2) > 0).all()
    # teacher-forced single sweep from random states at full length
    rng = np.random.default_rng(3)
    X0 = rng.integers(0, K, size=(W, T)).astype(np.int32)
    gt = _lib.estimate_batch_host(Y, Tw, K, 0, 1, (), None, x_init=X0, want_state=True)
    for w in range(W):
        o = oracle.estimate_window(Y[w], K, 0, 1, (), None, window_id=w, x_init=X0[w])
        assert_window_matches_oracle(gt, w, T, o, fields=("pif_final",), status0=False)


def test_signal_path_all_signal_real_data(hmclib, oracle, inflation):
    """estimatesignals! in the reference's committed "allsignal" configuration (code/run_hmm.jl:158-175): every
    position is a signal, HyperParams(opt) (alpha = nu = 2, kappa = noise), noise samples chained."""
    y, _ = inflation
    ends = [121, 122, 300]
    ld = max(ends)
    Y = np.zeros((3, ld)); Tw = np.array(ends, dtype=np.int32)
    for i, e in enumerate(ends):
        Y[i, :e] = y[:e]
    yreal = np.array([[y[e + 11]] for e in ends])
    sig = np.array([[0, e] for e in ends]); save = np.array([[e - 2, e] for e in ends])
    check_signals_against_oracle(oracle, Y, Tw, 3, 6, 15, 4, sig, save, 0.3, 2.0, 2.0, np.array([2.6, 2.5, 1.9]), yreal)
    # the base run inside estimatesignals! (:869-872): one chain, no noise, HyperParams(Y,D) with kappa = 1
    check_signals_against_oracle(oracle, Y, Tw, 3, 10, 30, 1, sig, save, 1.0, 1.0, 1.0, np.zeros(3), yreal)


def test_signal_path_partial_signal_synthetic(hmclib, oracle):
    """Signals on the tail of the window only (two populations in the conjugate update), K = 2 and 3, L = 1..4."""
    for K, T in ((3, 1000), (2, 300), (3, 500), (4, 600)):
        Y, Tw, fut = synth.generate_panel(3, T, K)
        sig = np.array([[T - 40, T], [T - 1, T], [T // 2, T]]); save = np.array([[T - 3, T], [T - 1, T], [T - 2, T]])
        check_signals_against_oracle(oracle, Y, Tw, K, 3, 8, 3, sig, save, 0.6, 2.0, 2.0, np.array([0.5, 1.0, 0.2]), fut[:, 11:12])


@pytest.mark.parametrize("K,T,sigLen", [(3, 300, 1), (3, 1000, 12), (2, 200, 3), (3, 140, 32), (3, 600, 48), (4, 700, 200), (2, 900, 256)])
def test_signal_path_signals_past_the_end_date(hmclib, oracle, K, T, sigLen):
    """estimatesignals! with sigLen = last(signalRange) - endIndex > 0 (src/Hmc.jl:888; the len_1 / len_12 runs of
    code/run_hmm.jl:122-158): pi_end reports the smoothed probabilities at endIndex (:900), horizon sigLen goes
    through forecastsignal (:908-909), a longer one is forecast h - sigLen steps from the last step (:906-907).
    No committed reference output covers this case: pinned by the oracle restatement only."""
    W = 3
    Y, Tw, fut = synth.generate_panel(W, T, K)
    Tw = np.array([T, T - 7, T - 64 if T > 200 else T - 1], dtype=np.int32)
    sig = np.stack([Tw - sigLen, Tw], axis=1).astype(np.int32)
    save = sig.copy()
    end_pos = (Tw - 1 - sigLen).astype(np.int32)
    ssig = np.array([0.4, 1.3, 0.05])
    horizons = (0, 12)                           # device horizons: slot 0 is the blend (h == sigLen), slot 1 is h = sigLen + 12
    yreal = np.stack([fut[:, 0], fut[:, 11]], axis=1)
    check_tail_signals_against_oracle(oracle, Y, Tw, K, 4, 10, 3, sig, save, ssig, end_pos, horizons, yreal, sigLen)
    # end_pos at the last step is the plain path, bit for bit
    a = _lib.estimate_batch_host(Y, Tw, K, 4, 10, (12,), yreal[:, 1:], sig_range=sig, sigma_signal=ssig, kappa=0.6, n_samples=2,
                                 end_pos=Tw - 1)
    b = _lib.estimate_batch_host(Y, Tw, K, 4, 10, (12,), yreal[:, 1:], sig_range=sig, sigma_signal=ssig, kappa=0.6, n_samples=2)
    assert_same(a, b, ("mu", "pi_end", "fcast", "summary"), equal_nan=False)
    # a tail longer than HMCG_MAXTAIL is flagged, not computed
    bad = _lib.estimate_batch_host(Y, Tw, K, 1, 2, (12,), yreal[:, 1:], sig_range=sig, sigma_signal=ssig, kappa=0.6,
                                   end_pos=Tw - 1 - (_lib.HMCG_MAXTAIL + 1))
    assert (bad["status"] == _lib.ST_BAD_T).all()


@pytest.mark.parametrize("K,lens", [(3, [1000, 257, 64, 5]), (2, [300, 2, 129]), (4, [700, 100, 3]),
                                    (5, [600, 65, 2, 300]), (8, [5000, 4999, 700]), (3, [5000, 4100]), (4, [1500, 1025])])
def test_smoothed_probabilities_mean(hmclib, oracle, K, lens):
    """Optional output: the draw-average of the smoothed probabilities pib[:, t, :] (backwardupdate_P!,
    src/Hmc.jl:442-457, sorted labels :513).  The GPU runs the beta recursion as a suffix scan; the oracle
    runs the reference's Pb recursion.  Same bar: 1e-9 on probabilities.  K <= 4 within the register-resident range
    runs the SMOOTH variants of gibbs_device.hpp; K >= 5 (incl. configs[3]'s 8 states, T = 5000) and longer windows run
    the smoothing variant of the LDS-resident kernel, which streams the running sums through HBM."""
    Y, Tw, fut = synth.generate_panel(len(lens), max(lens), K, ragged=lens)
    nrun = 12 if max(lens) <= 1000 else 5
    g = _lib.estimate_batch_host(Y, Tw, K, 3, nrun, (12,), fut[:, 11:12], want_state=True, want_smooth=True, want_filter_mean=True)
    for w in range(len(lens)):
        o = oracle.estimate_window(Y[w, :Tw[w]], K, 3, nrun, (12,), fut[w, 11:12], window_id=w, want_smooth=True)
        assert_window_matches_oracle(g, w, Tw[w], o, fields=("pi_smooth_mean", "pif_final", "mu"), status0=False)
        got = g["pi_smooth_mean"][w, :Tw[w]]                    # (T, K)
        assert np.max(np.abs(g["pi_filter_mean"][w, :Tw[w]].sum(axis=1) - 1)) < 1e-12
        assert np.max(np.abs(got.sum(axis=1) - 1)) < 1e-12
        assert np.max(np.abs(got[-1] - g["pi_end"][w].mean(axis=1))) < 1e-12       # pib[end,:] = pif[end,:] (:448)


def test_filtered_probability_mean_and_reference_insample_fixture(hmclib, oracle, inflation):
    """extras.pi_filter_mean: the draw average of the label-sorted filtered probabilities.  (1) against the oracle's
    running mean: 1e-9; flavours bit-identical.  (2) at the scale of the reference's committed
    official_insample/forecats_insample.csv (20k + 10k sweeps on 1970-01..2017-12, K = 3): its s1..s3 columns, which
    are these probabilities (see the oracle test of the same name for the tolerances)."""
    import csv
    import os
    y, dates = inflation
    Y = y[None, :576]
    Tw = np.array([576], dtype=np.int32)
    g = _lib.estimate_batch_host(Y, Tw, 3, 30, 60, (12,), np.array([[y[587]]]), want_filter_mean=True, want_smooth=True)
    o = oracle.estimate_signals(y[:576], 3, 30, 60, 1, horizons=(12,), yreal=[y[587]], want_filter_mean=True)
    assert_window_matches_oracle(g, 0, 576, o, fields=("pi_filter_mean",), status0=False, states=False)
    only = _lib.estimate_batch_host(Y, Tw, 3, 30, 60, (12,), np.array([[y[587]]]), want_filter_mean=True)    # without the smoother output
    assert np.array_equal(only["pi_filter_mean"], g["pi_filter_mean"]) and np.array_equal(only["mu"], g["mu"])
    rows = list(csv.DictReader(open(os.path.join(os.path.dirname(__file__), "golden", "official_insample_forecats_insample.csv"))))
    s = np.array([[float(r["s1"]), float(r["s2"]), float(r["s3"])] for r in rows])
    big = _lib.estimate_batch_host(Y, Tw, 3, 20000, 10000, (12,), np.array([[y[587]]]), want_filter_mean=True)
    d = np.abs(big["pi_filter_mean"][0] - s)
    assert d.mean() < 0.02 and d.max() < 0.3
    assert min(np.corrcoef(big["pi_filter_mean"][0][:, k], s[:, k])[0, 1] for k in range(3)) > 0.99
    # (3) the fixture's `forecast` column, to first order (see the oracle test): mean_j pif_j[t,:] . mean_j A_j^12 mu_j
    fc = np.array([float(r["forecast"]) for r in rows])
    A12 = np.linalg.matrix_power(np.transpose(big["A"][0], (2, 1, 0)), 12)
    c = np.einsum("nij,nj->ni", A12, big["mu"][0].T).mean(axis=0)
    f1 = big["pi_filter_mean"][0] @ c
    assert np.abs(f1 - fc).mean() < 0.07 and np.abs(f1 - fc).max() < 0.7 and np.corrcoef(f1, fc)[0, 1] > 0.997


def test_mixed_lengths_in_one_call(hmclib, oracle):
    lens = [1000, 17, 400, 2]
    Y, Tw, fut = synth.generate_panel(4, 1000, 3, ragged=lens)
    check_against_oracle(oracle, Y, Tw, 3, 2, 10, (1, 12), fut[:, [0, 11]])


def test_teacher_forced_single_sweep(hmclib, oracle):
    """Given the same X, one sweep: parameter draws, the whole filtered-probability path and the
    redrawn states must agree (this isolates the deterministic kernels from chain history)."""
    rng = np.random.default_rng(11)
    W, T, K = 6, 1000, 3
    Y, Tw, _ = synth.generate_panel(W, T, K)
    X0 = rng.integers(0, K, size=(W, T)).astype(np.int32)
    check_teacher_forced_against_oracle(oracle, Y, Tw, K, X0)


def test_real_data_expanding_windows(hmclib, oracle, inflation):
    y, _ = inflation
    ends = [120, 121, 250, 579]
    ld = max(ends)
    Y = np.zeros((len(ends), ld)); Tw = np.array(ends, dtype=np.int32)
    yreal = np.full((len(ends), 1), np.nan)
    for i, e in enumerate(ends):
        Y[i, :e] = y[:e]
        if e + 12 <= len(y):
            yreal[i, 0] = y[e + 11]
    check_against_oracle(oracle, Y, Tw, 3, 20, 60, (12,), yreal)


def test_status_flags(hmclib, oracle):
    Y, Tw, _ = synth.generate_panel(3, 300, 3)
    Y[1, 10] = np.nan                       # non-finite input
    Tw[2] = 1                               # too short
    g = _lib.estimate_batch_host(Y, Tw, 3, 2, 5, (12,), None, want_state=True)
    assert g["status"][0] == 0
    assert g["status"][1] == _lib.ST_NONFINITE
    assert g["status"][2] == _lib.ST_BAD_T
    assert np.isnan(g["mu"][1:]).all() and np.isnan(g["summary"][1:]).all()    # skipped windows read NaN, not a plausible zero
    # the C ABI itself hands back zeros for a skipped window (include/hmcg.h), whatever an earlier call left in the library's
    # recycled chunk buffers; the NaN is the Python layer's
    Yok, Tok, _ = synth.generate_panel(3, 300, 3)
    _lib.estimate_batch_host(Yok, Tok, 3, 0, 40, (12,), None)                                # leaves its draws in the chunk buffers
    raw = _lib.estimate_batch_host(Y, Tw, 3, 0, 40, (12,), None, nan_fill=False, want_corr=True)
    for k in ("mu", "sig2", "A", "pi_end", "fcast", "summary", "corr"):
        assert not raw[k][1:].any(), k
    assert np.isfinite(raw["mu"][0]).all() and raw["mu"][0].any()
    Tbad = Tw.copy(); Tbad[0] = 301                       # longer than the panel row (ldY = 300)
    assert _lib.estimate_batch_host(Y, Tbad, 3, 2, 5, (12,), None)["status"][0] == _lib.ST_BAD_T
    xbad = np.full((3, 300), 7, dtype=np.int32)            # out-of-range initial states are clamped, not trusted
    gb = _lib.estimate_batch_host(Y[:1], Tw[:1], 3, 0, 3, (12,), None, x_init=xbad[:1])
    assert gb["status"][0] == 0 and np.isfinite(gb["mu"]).all()
    # Emission underflow (the reference would produce NaN and throw, src/Hmc.jl:435): teacher-force every
    # point, including one 1e6 outlier, into state 0 of a long window.  sd_0 ~ 1e6/sqrt(T) puts the outlier
    # 55 sd out, the empty states' prior draws put it ~1e6 sd out: all K pdfs underflow at that step.
    T = 3000
    Yu, _, _ = synth.generate_panel(1, T, 3)
    Yu[0, 1500] = 1e6
    x0 = np.zeros((1, T), dtype=np.int32)
    gu = _lib.estimate_batch_host(Yu, [T], 3, 0, 1, (12,), None, x_init=x0, want_state=True)
    o = oracle.estimate_window(Yu[0], 3, 0, 1, (12,), None, x_init=x0[0])
    assert o["status"] & 2 and gu["status"][0] & _lib.ST_EMIS_UNDERFLOW
    assert np.array_equal(gu["x_final"][0], o["x_final"])
    assert close(gu["mu"][0].T, o["mu"]) < TOL and close(gu["pif_final"][0], o["pif_final"]) < TOL
    assert np.isfinite(gu["mu"][0]).all() and np.isfinite(gu["pif_final"][0]).all()
    # windows beyond the LDS are no longer refused (they stream through HBM: test_windows_beyond_the_lds_stream_through_hbm);
    # what still has no kernel: more than HMCG_MAXK states, and a thread count the LDS-resident kernel does not offer
    with pytest.raises(_lib.HmcgError):
        _lib.estimate_batch_host(np.zeros((1, 100)), [100], 9, 1, 1)
    with pytest.raises(_lib.HmcgError, match="no kernel"):
        _lib.estimate_batch_host(np.zeros((1, 20000)), [20000], 3, 1, 1, threads_per_window=512)


def test_sharding_reproduces_unsharded_rows(hmclib):
    """Explicit RNG stream ids: any subset of windows, in any order, on its own call equals the
    same rows of the full run bit for bit (what makes the multi-GPU split invisible)."""
    Y, Tw, fut = synth.generate_panel(12, 500, 3)
    full = _lib.estimate_batch_host(Y, Tw, 3, 5, 30, (12,), fut[:, 11:12], want_state=True)
    ids = np.array([7, 2, 11])
    part = _lib.estimate_batch_host(Y[ids], Tw[ids], 3, 5, 30, (12,), fut[ids, 11:12], want_state=True, window_ids=ids)
    for k in ("mu", "sig2", "A", "pi_end", "fcast", "summary", "x_final", "pif_final"):
        assert np.array_equal(part[k], full[k][ids]), k
    based = _lib.estimate_batch_host(Y[4:8], Tw[4:8], 3, 5, 30, (12,), fut[4:8, 11:12], window_base=4)
    assert np.array_equal(based["mu"], full["mu"][4:8])


def test_checkpoint_resume_is_exact(hmclib):
    """12+28 sweeps in one call == 15 sweeps, checkpoint (xstate, sumacc, status), resume 25."""
    Y, Tw, fut = synth.generate_panel(5, 700, 3)
    one = _lib.estimate_batch_host(Y, Tw, 3, 12, 28, (12,), fut[:, 11:12], want_state=True)
    a = _lib.estimate_batch_host(Y, Tw, 3, 12, 28, (12,), fut[:, 11:12], want_state=True, sweep_count=15)
    b = _lib.estimate_batch_host(Y, Tw, 3, 12, 28, (12,), fut[:, 11:12], resume_state=a, sweep_base=15)
    assert np.array_equal(a["mu"][:, :, :3], one["mu"][:, :, :3])          # draws 0..2 came from the first call
    assert np.array_equal(b["mu"][:, :, 3:], one["mu"][:, :, 3:])          # the rest from the resumed one
    assert np.array_equal(b["A"][..., 3:], one["A"][..., 3:])
    assert np.array_equal(b["summary"], one["summary"])
    assert np.array_equal(b["xstate"][:, :700], one["x_final"].astype(np.uint8))


def test_signal_run_resumed_inside_a_noise_sample(hmclib):
    """extras.sample_summary across a checkpoint: 3 noise samples of 4 + 9 sweeps; the first call stops after 19 sweeps
    (sample 1, two of its kept draws done), the RESUME call finishes.  The per-sample rows of the pair must equal the
    single call's: the row of an unfinished sample carries its raw running sums from one call to the next."""
    K, T, W = 3, 400, 4
    Y, Tw, fut = synth.generate_panel(W, T, K)
    sig = np.stack([Tw - 25, Tw], axis=1).astype(np.int32)
    kw = dict(sig_range=sig, save_range=sig, sigma_signal=np.array([0.4, 0.9, 0.1, 0.6]), kappa=0.6, n_samples=3, alpha=2.0, nu=2.0,
              want_sample_summary=True)
    one = _lib.estimate_batch_host(Y, Tw, K, 4, 9, (12,), fut[:, 11:12], want_state=True, **kw)
    a = _lib.estimate_batch_host(Y, Tw, K, 4, 9, (12,), fut[:, 11:12], want_state=True, sweep_count=19, **kw)
    assert np.array_equal(a["sample_summary"][:, 0], one["sample_summary"][:, 0])                # sample 0 complete
    b = _lib.estimate_batch_host(Y, Tw, K, 4, 9, (12,), fut[:, 11:12], resume_state=a, sweep_base=19,
                                 resume_sample_summary=a["sample_summary"], **kw)
    assert np.array_equal(b["sample_summary"], one["sample_summary"]) and np.array_equal(b["summary"], one["summary"])
    # and the rows average to the whole-run summary (equal sample sizes)
    assert np.max(np.abs(one["sample_summary"].mean(axis=1) - one["summary"])) < 1e-12


def test_signal_run_resumed_with_every_running_sum(hmclib):
    """The chain above split at the same place, now carrying everything a RESUME call reads back at once -- xstate, sumacc,
    status, sample_summary and the running smoothed / filtered means (the Python wrapper does not carry the last two, so
    the calls go through the C ABI).  The pair must equal the single call bit for bit."""
    import ctypes as C
    K, T, W, burnin, nrun, n_samples, H = 3, 400, 4, 4, 9, 3, 1
    NS = 3 * K + K * K + 2 * H
    Y, Tw, fut = synth.generate_panel(W, T, K)
    Y, Tw32, yreal = np.ascontiguousarray(Y, np.float64), np.ascontiguousarray(Tw, np.int32), np.ascontiguousarray(fut[:, 11:12])
    sig = np.ascontiguousarray(np.stack([Tw - 25, Tw], axis=1).astype(np.int32))
    sigma = np.array([0.4, 0.9, 0.1, 0.6])
    L = _lib.load()
    carried = ("status", "xstate", "sumacc", "sample_summary", "pi_smooth_mean", "pi_filter_mean")

    def call(flags, sweep_base, sweep_count, state=None):
        o = dict(status=np.zeros(W, np.int32), xstate=np.zeros((W, T), np.uint8), sumacc=np.zeros((W, NS + K)),
                 sample_summary=np.zeros((W, n_samples, NS)), pi_smooth_mean=np.zeros((W, T, K)), pi_filter_mean=np.zeros((W, T, K)))
        if state is not None:
            o = {k: state[k].copy() for k in carried}
        o["summary"] = np.zeros((W, NS))
        o["mu"] = np.zeros((W, K, n_samples * nrun))
        ex = _lib.Extras()
        ex.struct_size = C.sizeof(_lib.Extras)
        ex.sig_range, ex.sigma_signal = sig.ctypes.data, sigma.ctypes.data
        for k in carried[1:]:
            setattr(ex, k, o[k].ctypes.data)
        cfg = _lib.make_config(W, K, T, T, burnin, nrun, (12,), flags=flags, sweep_base=sweep_base, alpha=2.0, nu=2.0,
                               sweep_count=sweep_count, kappa=0.6, n_samples=n_samples)
        p = _lib._np_ptr
        rc = L.hmcg_estimate_batch(C.byref(cfg), p(Y), p(Tw32), p(yreal), p(o["mu"]), None, None, None, None, p(o["summary"]),
                                   p(o["status"]), C.byref(ex), None)
        assert rc == 0, L.hmcg_last_error()
        return o

    one = call(0, 0, 0)
    a = call(0, 0, 19)
    b = call(_lib.FLAG_RESUME, 19, 0, a)
    for k in carried + ("summary",):
        assert np.array_equal(b[k], one[k]), k
    d = nrun + 2                   # kept draws of the first 19 sweeps: sample 0, then two of sample 1
    assert np.array_equal(a["mu"][:, :, :d], one["mu"][:, :, :d]) and np.array_equal(b["mu"][:, :, d:], one["mu"][:, :, d:])


# (K, L, NT) of the kernel rows with a thread count of their own (csrc/variants_k3.hip), each selected by threads_per_window=NT
# at T = 1000; tests/test_variant_coverage.py holds this list to the tables
THREADS_PER_WINDOW_CASES = [(3, 8, 128), (3, 2, 512)]


def test_threads_per_window_variants_agree(hmclib, oracle):
    """The 128- and 512-thread decompositions scan in a different association order; they must
    still match the oracle (and hence each other) within tolerance with identical state paths."""
    for K, L, tpw in THREADS_PER_WINDOW_CASES:
        Y, Tw, fut = synth.generate_panel(3, 1000, K)
        g = check_against_oracle(oracle, Y, Tw, K, 2, 20, (12,), fut[:, 11:12], threads_per_window=tpw)
        assert g["threads_per_window"] == tpw and g["steps_per_thread"] == L and g["buckets"] == 1


@pytest.mark.parametrize("K", [2, 3, 4])
def test_kernel_flavours_are_bit_identical(hmclib, monkeypatch, K):
    """Each kernel variant exists in three flavours -- plain, plain with registers capped so that two windows
    share a CU, and with four helper waves per window (draw-phase jobs off the window's own threads) -- and
    the library picks by batch size.  All do the same arithmetic on the same counter-based random numbers,
    so every output must agree bit for bit: on every steps-per-thread variant, on the signal path and with
    the smoothed-probability output."""
    lens = [5, 200, 256, 500, 1000, 2047]
    Y, Tw, fut = synth.generate_panel(len(lens), max(lens), K, ragged=lens)
    for sub in ([0, 1, 2], [3], [4], [5]):
        idx = np.array(sub)
        ld = int(Tw[idx].max())
        args = (np.ascontiguousarray(Y[idx, :ld]), Tw[idx], K, 3, 12, (3, 12, 40),
                np.column_stack([fut[idx, 2], fut[idx, 11], np.zeros(len(idx))]))      # h=40 takes the long-horizon branch
        extra = [dict()]
        if ld <= 1024:
            sig = np.stack([np.maximum(Tw[idx] - 12, 0), Tw[idx]], axis=1).astype(np.int32)
            extra += [dict(sig_range=sig, kappa=1.0, n_samples=2, sigma_signal=np.full(len(idx), 0.3)), dict(want_smooth=True, want_filter_mean=True)]
        for kw in extra:
            res = {}
            for fl in ("p1", "p2", "h"):       # plain / plain capped for two blocks per CU / helper waves
                monkeypatch.setenv("HMCG_FLAVOUR", fl)
                res[fl] = _lib.estimate_batch_host(*args, want_state=True, window_ids=idx, **kw)
            assert res["h"]["helper_waves"] == 4 and res["p1"]["helper_waves"] == 0
            for fl in ("p2", "h"):
                a, b = res["p1"], res[fl]
                assert_same(a, b, DRAWS + ("x_final", "pif_final", "status"), what=(K, sub, sorted(kw), fl))
                if "want_smooth" in kw:
                    assert_same(a, b, ("pi_smooth_mean", "pi_filter_mean"), equal_nan=False)


def test_batch_larger_than_the_gpu_matches_small_batches(hmclib):
    """More windows than CUs switches the library to the two-windows-per-CU kernels; rows must not depend on
    the batch they were computed in."""
    W = 600
    Y, Tw, fut = synth.generate_panel(W, 300, 3)
    big = _lib.estimate_batch_host(Y, Tw, 3, 2, 6, (12,), fut[:, 11:12], want_state=True)
    assert big["helper_waves"] == 0
    ids = np.array([0, 299, 300, 599])
    small = _lib.estimate_batch_host(Y[ids], Tw[ids], 3, 2, 6, (12,), fut[ids, 11:12], want_state=True, window_ids=ids)
    assert small["helper_waves"] == 4
    for k in ("mu", "sig2", "A", "pi_end", "fcast", "summary", "x_final", "pif_final", "status"):
        assert np.array_equal(big[k][ids], small[k]), k


def test_full_size_cfg2_properties_and_subset_parity(hmclib, oracle):
    """BASELINE configs[1] at full size (256 windows, T=1000, 1000 draws): size-independent
    properties on everything, oracle parity on a subset of windows at full length."""
    W, T, K, n = 256, 1000, 3, 1000
    Y, Tw, fut = synth.generate_panel(W, T, K)
    yreal = fut[:, 11:12]
    g = _lib.estimate_batch_host(Y, Tw, K, 0, n, (12,), yreal, want_state=True)
    assert (g["status"] == 0).all()
    mu = np.transpose(g["mu"], (0, 2, 1)); A = np.transpose(g["A"], (0, 3, 2, 1)); pe = np.transpose(g["pi_end"], (0, 2, 1))
    assert (np.diff(mu, axis=2) > 0).all()                                     # labels sorted on every draw
    assert np.max(np.abs(A.sum(axis=3) - 1)) < 1e-12 and (A > 0).all()         # row-stochastic
    assert np.max(np.abs(pe.sum(axis=2) - 1)) < 1e-12
    assert (g["sig2"] > 0).all() and np.isfinite(g["fcast"]).all()
    assert np.max(np.abs(g["pif_final"].sum(axis=2) - 1)) < 1e-12              # every filtered law is a simplex point
    assert g["x_final"].min() >= 0 and g["x_final"].max() < K
    # forecast identity and error column, recomputed on the host from the returned draws
    A12 = np.linalg.matrix_power(A[:8], 12)
    f = np.einsum("wdr,wdrs,wds->wd", pe[:8], A12, mu[:8])
    assert np.max(np.abs(f - g["fcast"][:8, 0, :])) < 1e-9
    assert np.max(np.abs(g["fcast"][:, 1, :] - (g["fcast"][:, 0, :] - yreal))) < 1e-12
    # summary = mean over draws of round(x, 5) in the documented row order
    rows = np.concatenate([g["mu"], g["sig2"], g["pi_end"], g["A"].reshape(W, K * K, n), g["fcast"]], axis=1)
    ref = (np.rint(rows * 1e5) / 1e5).mean(axis=2)
    assert np.max(np.abs(ref - g["summary"])) < 1e-10
    # determinism: a second run is bitwise identical
    g2 = _lib.estimate_batch_host(Y, Tw, K, 0, n, (12,), yreal, want_state=True)
    assert_same(g, g2, FLOAT_KEYS + ("x_final",), equal_nan=False)
    # oracle parity on 6 windows at full size
    ids = np.array([0, 1, 37, 128, 200, 255])
    for w in ids:
        o = oracle.estimate_window(Y[w], K, 0, n, (12,), yreal[w], window_id=int(w))
        assert_window_matches_oracle(g, w, T, o, fields=("mu", "sig2", "A", "fcast", "summary", "pif_final"))


def test_device_resident_entry_matches_host_entry(hmclib):
    from hmc_jl_amd.device import DevicePanel
    Y, Tw, fut = synth.generate_panel(16, 600, 3)
    host = _lib.estimate_batch_host(Y, Tw, 3, 4, 25, (12,), fut[:, 11:12])
    p = DevicePanel(Y, Tw, 3, 25, (12,), fut[:, 11:12])
    ms = p.run(burnin=4)
    assert ms > 0
    for k in ("mu", "sig2", "A", "pi_end", "fcast", "summary"):
        assert np.array_equal(getattr(p, k).cpu().numpy(), host[k]), k
    assert (p.status.cpu().numpy() == 0).all()
    p.run(burnin=4, timed=False)            # asynchronous form
    p.sync()
    assert np.array_equal(p.summary.cpu().numpy(), host["summary"])


@pytest.mark.parametrize("idx,date", [(120, "1979-12-01"), (350, "1999-02-01"), (579, "2018-03-01")])
def test_gpu_posterior_vs_reference_committed_summaries(hmclib, inflation, golden_summaries, idx, date):
    """Statistical agreement of the GPU chain with the reference's own committed outputs
    (data/output/official/*_summary.csv: 100k burn-in + 250k draws upstream; here 10k + 100k)."""
    y, _ = inflation
    yreal = np.array([[y[idx + 11]]]) if idx + 12 <= len(y) else None
    g = _lib.estimate_batch_host(y[None, :idx], [idx], 3, 10000, 100000, (12,), yreal, want_draws=False)
    s = g["summary"][0]
    K = 3
    assert g["status"][0] == 0
    np.testing.assert_allclose(s[0:K], golden_summaries["filtered_means"][1][date], atol=0.04)
    np.testing.assert_allclose(s[K:2 * K], golden_summaries["filtered_variances"][1][date], atol=0.08, rtol=0.02)
    np.testing.assert_allclose(s[2 * K:3 * K], golden_summaries["filtered_state_probs"][1][date], atol=0.002)
    np.testing.assert_allclose(s[3 * K:3 * K + K * K], golden_summaries["filtered_trans_probs"][1][date], atol=0.003)
    np.testing.assert_allclose(s[3 * K + K * K], golden_summaries["forecasts"][1][date][0], atol=0.03)


def test_gpu_reference_unit_test_truth_recovery(hmclib):
    """test/runtests.jl:20-57 on the GPU path: 2-state, 476 of 500 points, 3000 + 1000 sweeps."""
    Y, _ = synth.generate_window(500, 2, seed=126)
    g = _lib.estimate_batch_host(Y[None, :476], [476], 2, 3000, 1000, (12,), np.array([[Y[487]]]))
    np.testing.assert_allclose(g["mu"][0].mean(axis=1), [-5.0, 4.0], atol=0.3)
    np.testing.assert_allclose(g["sig2"][0].mean(axis=1), [1.0, 0.5], atol=0.5)


def test_full_size_cfg4_properties_and_subset_identity(hmclib, oracle):
    """BASELINE configs[3] at full size (8 states, T=5000, 512 windows; 12 draws instead of 1000): size-independent
    properties on every window, batching invariance against the same windows run on their own with their global ids (bit
    for bit -- the pdf scratch, the chunk products and the maps are per window), oracle parity on one window."""
    W, T, K, n = 512, 5000, 8, 12
    Y, Tw, fut = synth.generate_panel(W, T, K)
    yreal = fut[:, 11:12]
    g = _lib.estimate_batch_host(Y, Tw, K, 3, n, (12,), yreal, want_state=True)
    assert (g["status"] == 0).all() and g["steps_per_thread"] == 20
    mu = np.transpose(g["mu"], (0, 2, 1)); A = np.transpose(g["A"], (0, 3, 2, 1)); pe = np.transpose(g["pi_end"], (0, 2, 1))
    assert (np.diff(mu, axis=2) > 0).all()
    assert np.max(np.abs(A.sum(axis=3) - 1)) < 1e-12 and (A > 0).all()
    assert np.max(np.abs(pe.sum(axis=2) - 1)) < 1e-12 and (g["sig2"] > 0).all() and np.isfinite(g["fcast"]).all()
    assert np.max(np.abs(g["pif_final"].sum(axis=2) - 1)) < 1e-12
    assert g["x_final"].min() >= 0 and g["x_final"].max() < K
    rows = np.concatenate([g["mu"], g["sig2"], g["pi_end"], g["A"].reshape(W, K * K, n), g["fcast"]], axis=1)
    assert np.max(np.abs((np.rint(rows * 1e5) / 1e5).mean(axis=2) - g["summary"])) < 1e-10
    ids = np.array([0, 255, 256, 511])                      # first and second round of windows on the 256 CUs
    sub = _lib.estimate_batch_host(np.ascontiguousarray(Y[ids]), Tw[ids], K, 3, n, (12,), yreal[ids], want_state=True, window_ids=ids)
    for k in FLOAT_KEYS + ("x_final",):
        assert np.array_equal(g[k][ids], sub[k]), k
    o = oracle.estimate_window(Y[511], K, 3, n, (12,), yreal[511], window_id=511)
    assert_window_matches_oracle(g, 511, T, o, fields=("mu", "A", "fcast", "pif_final"))


@pytest.mark.parametrize("K,lens", [(3, [20000, 7600, 12001]), (8, [8000, 6700]), (5, [9000]), (2, [30000])])
def test_windows_beyond_the_lds_stream_through_hbm(hmclib, oracle, K, lens):
    """Windows longer than a CU's LDS holds (about 5 500 steps at K = 8, 6 000 at K = 3) used to be refused (`no kernel`,
    VERDICT r2 missing #2); the reference's loops are unbounded in N (src/Hmc.jl:406).  They now run on the streaming form
    of the LDS-resident kernel (per-step arrays in an HBM scratch): same oracle parity as everywhere else."""
    Y, Tw, fut = synth.generate_panel(len(lens), max(lens), K, ragged=lens)
    g = check_against_oracle(oracle, Y, Tw, K, 1, 3, (1, 12), fut[:, [0, 11]])
    assert (g["status"] == 0).all() and g["streaming"] and g["steps_per_thread"] == (max(lens) + 255) // 256


@pytest.mark.parametrize("K,lens", [(8, [5000, 4999, 700, 64]), (3, [4100, 2500]), (6, [3000, 1, 2])])
def test_streaming_form_equals_the_lds_resident_kernel(hmclib, monkeypatch, K, lens):
    """HMCG_FORCE_STREAM runs the streaming form where the LDS-resident one would do: the two are the same code over two
    address spaces, so every output is bit-identical -- chunked launches and a resumed chain included."""
    lens = [t for t in lens if t >= 2]
    Y, Tw, fut = synth.generate_panel(len(lens), max(lens), K, ragged=lens)
    args = (Y, Tw, K, 3, 9, (1, 12), fut[:, [0, 11]])
    a = _lib.estimate_batch_host(*args, want_state=True)
    monkeypatch.setenv("HMCG_FORCE_STREAM", "1")
    monkeypatch.setenv("HMCG_CHUNK_DRAWS", "4")
    b = _lib.estimate_batch_host(*args, want_state=True)
    assert b["lds_bytes"] < a["lds_bytes"] and b["launches"] >= 2
    assert_same(a, b, DRAWS + ("status", "x_final", "pif_final"))


@pytest.mark.parametrize("K,T", [(8, 600), (5, 300), (6, 1500), (7, 257), (3, 3000), (4, 2500)])
def test_signal_path_on_the_lds_resident_kernel(hmclib, oracle, K, T):
    """estimatesignals! for D >= 5 (VERDICT r2 missing #1: the reference's loop works for any D, src/Hmc.jl:868-914) and for
    K <= 4 windows beyond the register-resident SIG variants: the SIG form of the LDS-resident kernel -- two-population
    statistics, (1 + kappa) signal emission sd, chained noise samples, per-sample summaries."""
    Y, Tw, fut = synth.generate_panel(3, T, K)
    Tw = np.array([T, T - 3, max(T // 2, 8)], dtype=np.int32)
    sig = np.array([[Tw[0] - 40, Tw[0]], [Tw[1] - 1, Tw[1]], [0, Tw[2]]])             # a tail, one step, everything a signal
    save = np.array([[Tw[0] - 3, Tw[0]], [Tw[1] - 1, Tw[1]], [Tw[2] - 2, Tw[2]]])
    g = check_signals_against_oracle(oracle, Y, Tw, K, 3, 7, 3, sig, save, 0.6, 2.0, 2.0, np.array([0.5, 1.0, 0.2]), fut[:, 11:12])
    assert g["steps_per_thread"] == (T + 255) // 256 and g["helper_waves"] == 0
    # the base run inside estimatesignals! (:869-872): one chain, no noise, HyperParams(Y,D) with kappa = 1
    check_signals_against_oracle(oracle, Y, Tw, K, 4, 9, 1, sig, save, 1.0, 1.0, 1.0, np.zeros(3), fut[:, 11:12])


@pytest.mark.parametrize("K,T,sigLen", [(8, 400, 48), (5, 700, 1), (6, 300, 12), (3, 2600, 200)])
def test_signals_past_the_end_date_on_the_lds_resident_kernel(hmclib, oracle, monkeypatch, K, T, sigLen):
    """sigLen > 0 at K = 8 with 48 signal steps (VERDICT r2 item 7's example): smoothed probabilities at endIndex (:900) from the
    beta recursion over the tail's emission values (read back from the pdf scratch), forecastsignal for h == sigLen (:908-909).
    Also through the HBM-streaming form, bit for bit."""
    W = 3
    Y, Tw, fut = synth.generate_panel(W, T, K)
    Tw = np.array([T, T - 7, T - 64], dtype=np.int32)
    sig = np.stack([Tw - sigLen, Tw], axis=1).astype(np.int32)
    end_pos = (Tw - 1 - sigLen).astype(np.int32)
    ssig = np.array([0.4, 1.3, 0.05])
    horizons = (0, 12)
    yreal = np.stack([fut[:, 0], fut[:, 11]], axis=1)
    kw = dict(sig_range=sig, save_range=sig, sigma_signal=ssig, kappa=0.6, n_samples=3, alpha=2.0, nu=2.0, end_pos=end_pos, blend_mask=1,
              want_sample_summary=True)
    g = check_tail_signals_against_oracle(oracle, Y, Tw, K, 4, 10, 3, sig, sig, ssig, end_pos, horizons, yreal, sigLen, want_sample_summary=True)
    monkeypatch.setenv("HMCG_FORCE_STREAM", "1")
    monkeypatch.setenv("HMCG_CHUNK_DRAWS", "7")
    s = _lib.estimate_batch_host(Y, Tw, K, 4, 10, horizons, yreal, want_state=True, **kw)
    assert_same(g, s, DRAWS + ("sample_summary", "sigvals", "x_final", "pif_final"))


@pytest.mark.parametrize("K,lens", [(3, [1000, 257, 64]), (2, [300, 2]), (4, [700, 100]), (8, [900, 300]), (5, [600, 65]), (3, [5000]), (3, [8000])])
def test_per_draw_smoothed_probabilities(hmclib, oracle, monkeypatch, K, lens):
    """extras.pi_smooth_draws: the reference's samples.pib[Nrun, N, D] itself (gibbssample!, src/Hmc.jl:552,558) -- every kept
    draw's smoothed probabilities in sorted labels, [W][K][ldY][nd] = Julia (Nrun, N, D, W) -- from the register-resident SMOOTH
    variants, the LDS-resident smoothing kernel and its HBM-streaming form, against the oracle's literal Pb recursion;
    streamed by the host entry in chunks (a chunk size that does not divide the run), equal to the single launch."""
    Y, Tw, fut = synth.generate_panel(len(lens), max(lens), K, ragged=lens)
    burnin, nrun = 2, 7
    args = (Y, Tw, K, burnin, nrun, (12,), fut[:, 11:12])
    g = _lib.estimate_batch_host(*args, want_state=True, want_smooth_draws=True, want_smooth=True)
    for w in range(len(lens)):
        T = int(Tw[w])
        o = oracle.estimate_window(Y[w, :T], K, burnin, nrun, (12,), fut[w, 11:12], window_id=w, want_smooth=True)
        assert_window_matches_oracle(g, w, T, o, fields=("pi_smooth_draws",))
        got = np.transpose(g["pi_smooth_draws"][w, :, :T, :], (2, 1, 0))              # (nrun, T, K)
        assert np.max(np.abs(got.sum(axis=2) - 1)) < 1e-12
        assert np.max(np.abs(got[:, -1, :] - g["pi_end"][w].T)) < 1e-12              # pib[:, end, :] is what pi_end reports (:448)
        assert np.max(np.abs(got.mean(axis=0) - g["pi_smooth_mean"][w, :T])) < 1e-12
        assert not g["pi_smooth_draws"][w, :, T:, :].any()                            # beyond the window: untouched zeros
    monkeypatch.setenv("HMCG_CHUNK_DRAWS", "3")
    c = _lib.estimate_batch_host(*args, want_state=True, want_smooth_draws=True)
    assert c["launches"] >= 3 and np.array_equal(c["pi_smooth_draws"], g["pi_smooth_draws"]) and np.array_equal(c["mu"], g["mu"])


@pytest.mark.parametrize("K,lens", [(3, [1000, 999, 64, 7, 2, 513, 2050]), (2, [300, 301]), (4, [700, 1001]), (8, [900, 901, 5000]), (5, [64, 65])])
def test_median_selection_with_ties_and_signed_zeros(hmclib, oracle, K, lens):
    """The fresh start's median (makeParams, src/Hmc.jl:161-195) is a radix selection over integer keys (block_select,
    csrc/gibbs_device.hpp); the oracle sorts.  Data made of few distinct values -- quantised to one decimal, with runs of
    equal middle elements, exact zeros of both signs, even and odd T, windows of one value repeated but for two entries --
    must give the same initial state path and hence the same chain (state paths bit-exact) on both kernels."""
    rng = np.random.default_rng(42)
    W, ld = len(lens), max(lens)
    Y = np.zeros((W, ld))
    for w, T in enumerate(lens):
        y = np.round(rng.normal(0.0, 1.0, T) + (rng.random(T) < 0.3) * 2.0, 1)
        y[rng.random(T) < 0.15] = 0.0
        y[rng.random(T) < 0.10] = -0.0
        if w % 3 == 2 and T > 4:                       # nearly constant: the two middle elements are the same value
            y[:] = 0.5
            y[0], y[-1] = -1.0, 2.0
        Y[w, :T] = y
    Tw = np.array(lens, dtype=np.int32)
    yreal = rng.normal(0.0, 1.0, (W, 1))
    for lo in range(0, W, 3):                           # (the oracle is sequential: a few windows at a time)
        idx = np.arange(lo, min(lo + 3, W))
        l2 = int(Tw[idx].max())
        check_against_oracle(oracle, np.ascontiguousarray(Y[idx, :l2]), Tw[idx], K, 2, 6 if l2 > 2000 else 12, (12,), yreal[idx])
