"""One oracle-parity case for EVERY dispatchable kernel instantiation of csrc/variants_*.hip.

Each row of the variant tables (K, steps per thread L, path, flavour) is driven with a window long enough to select
exactly that row (256*(L/2) < T <= 256*L), forced to the flavour under test, run as a free chain for a few sweeps
and compared with the oracle: state paths bit-exact, floats within 1e-9 relative-to-(1+|x|).  The call's own
report (steps_per_thread, helper_waves) asserts that the intended instantiation ran.  VERDICT r1 item 2: the
spill-heavy neighbours of the round-1 fault (K=3 L=16 base, SIG/SMOOTH L=8) had no parity test."""
import numpy as np
import pytest

from hmc_jl_amd import _lib, synth
from kernel_tables import FLAVOUR_WAVES, SIGSMOOTH, VARIANT_CASES as CASES, VARIANT_ROWS as ROWS, steps_per_thread
from oracle_parity import FLOAT_KEYS, assert_window_matches_oracle

pytestmark = pytest.mark.gpu


def test_variant_tables_are_covered():
    """The parser sees every row (the counts are those of the tables; a new row is picked up automatically)."""
    assert len(ROWS) >= 33 and (3, 16, "base") in ROWS and (3, 8, "sig") in ROWS and (3, 8, "smooth") in ROWS


@pytest.mark.parametrize("K,L,path,flavour", CASES, ids=["K%d-L%d-%s-%s" % c for c in CASES])
def test_every_variant_against_oracle(hmclib, oracle, monkeypatch, K, L, path, flavour):
    monkeypatch.setenv("HMCG_FLAVOUR", flavour)
    Tmax = 256 * L - (1 if L > 1 else 0)               # odd length just under the variant's capacity (L=1: 256)
    Tmin = 256 * (L // 2) + 1 if L > 1 else 2          # shortest window that still selects this L
    lens = [Tmax, max(Tmin, Tmax - 129)]
    Y, Tw, fut = synth.generate_panel(2, Tmax, K, ragged=lens)
    burnin, nrun, horizons = 2, 5, (1, 12)
    yreal = fut[:, [0, 11]]
    ids = np.array([3, 8])
    if path == "sig":
        sig = np.stack([Tw - np.array([40, 1]), Tw], axis=1).astype(np.int32)
        save = np.stack([Tw - 2, Tw], axis=1).astype(np.int32)
        ssig = np.array([0.5, 1.0])
        g = _lib.estimate_batch_host(Y, Tw, K, burnin, nrun, horizons, yreal, want_state=True, window_ids=ids,
                                     sig_range=sig, save_range=save, sigma_signal=ssig, kappa=0.6, n_samples=2,
                                     alpha=2.0, nu=2.0)
    else:
        g = _lib.estimate_batch_host(Y, Tw, K, burnin, nrun, horizons, yreal, want_state=True, window_ids=ids,
                                     want_smooth=(path == "smooth"), want_filter_mean=(path == "smooth"))
    assert g["steps_per_thread"] == L and g["threads_per_window"] == 256, (g["steps_per_thread"], L)
    assert (g["helper_waves"], g["occupancy"]) == FLAVOUR_WAVES[flavour]   # the NH and OCC arguments of the three HMCG_V3 expansions
    assert g["buckets"] == (1 if steps_per_thread(K, lens[1], path == "sig", path == "smooth") == L else 2)     # 2: the second window falls a class lower
    for w in range(2):
        T = int(Tw[w])
        if path == "sig":
            o = oracle.estimate_signals(Y[w, :T], K, burnin, nrun, 2, sig=tuple(sig[w]), kappa=0.6, alpha=2.0, nu=2.0,
                                        sigma_signal=float(ssig[w]), save=tuple(save[w]), horizons=horizons,
                                        yreal=yreal[w], window_id=int(ids[w]))
        else:
            o = oracle.estimate_window(Y[w, :T], K, burnin, nrun, horizons, yreal[w], window_id=int(ids[w]),
                                       want_smooth=(path == "smooth"))
        assert_window_matches_oracle(g, w, T, o, fields=FLOAT_KEYS + {"sig": ("sigvals",), "smooth": ("pi_smooth_mean",), "base": ()}[path], nsave=2)


@pytest.mark.parametrize("T", [2049, 3000, 3073, 4096])
def test_k3_sixteen_steps_per_thread_lengths(hmclib, oracle, T):
    """K = 3, T in 2049..4096: the L = 12 (T <= 3072) and L = 16 register-resident kernels, default dispatch, longer chain
    than the per-variant sweep above; the second window (500 steps shorter) may fall into the class below: bucketed."""
    Y, Tw, fut = synth.generate_panel(2, T, 3, ragged=[T, T - 500])
    g = _lib.estimate_batch_host(Y, Tw, 3, 3, 12, (12,), fut[:, 11:12], want_state=True)
    assert g["steps_per_thread"] == (12 if T <= 3072 else 16)
    for w in range(2):
        o = oracle.estimate_window(Y[w, :Tw[w]], 3, 3, 12, (12,), fut[w, 11:12], window_id=w)
        assert_window_matches_oracle(g, w, Tw[w], o, status0=False)


def test_bad_signal_ranges_are_flagged_not_written(hmclib):
    """sig_range / save_range are caller data.  A save range longer than nsave_ld, a range outside the
    window, or a non-empty signal range that does not end at T must flag the window (HMCG_ST_BAD_RANGE) and write
    nothing -- not index past the sigvals slab."""
    import ctypes as C
    Y, Tw, fut = synth.generate_panel(3, 300, 3)
    L = _lib.load()
    W, K, nrun, ns, nsave = 3, 3, 4, 2, 2
    sig = np.array([[290, 300], [290, 300], [290, 299]], dtype=np.int32)       # window 2: does not end at T
    save = np.array([[290, 300], [298, 300], [298, 300]], dtype=np.int32)      # window 0: 10 positions into a 2-wide slab
    sentinel = -7.25
    flat = np.full(W * ns * nsave + 64, sentinel)                              # slack after the slabs to catch overruns
    out = {k: np.zeros(s) for k, s in dict(mu=(W, K, ns * nrun), summary=(W, 3 * K + K * K + 2)).items()}
    status = np.zeros(W, dtype=np.int32)
    ex = _lib.Extras(); ex.struct_size = C.sizeof(_lib.Extras)
    ssg = np.array([0.3, 0.3, 0.3])
    ex.sig_range = sig.ctypes.data; ex.save_range = save.ctypes.data; ex.sigma_signal = ssg.ctypes.data
    ex.sigvals = flat.ctypes.data; ex.nsave_ld = nsave
    cfg = _lib.make_config(W, K, 300, 300, 1, nrun, (12,), kappa=0.5, n_samples=ns)
    T32 = np.ascontiguousarray(Tw, dtype=np.int32)
    yr = np.ascontiguousarray(fut[:, 11:12])
    rc = L.hmcg_estimate_batch(C.byref(cfg), _lib._np_ptr(Y), _lib._np_ptr(T32), _lib._np_ptr(yr), _lib._np_ptr(out["mu"]),
                               None, None, None, None, _lib._np_ptr(out["summary"]), _lib._np_ptr(status), C.byref(ex), None)
    assert rc == 0
    assert status[0] == _lib.ST_BAD_RANGE and status[2] == _lib.ST_BAD_RANGE and status[1] == 0
    body = flat[:W * ns * nsave].reshape(W, ns, nsave)
    assert (flat[W * ns * nsave:] == sentinel).all()                           # nothing past the buffer
    assert (body[1] != sentinel).all() and (body[1] != 0).all()               # the valid window reported its values
    assert (out["mu"][0] == 0).all() and (out["mu"][2] == 0).all() and (out["mu"][1] != 0).all()
    # ... and exactly the values a call with that window alone reports (no neighbour wrote into its slab)
    alone = _lib.estimate_batch_host(Y[1:2], Tw[1:2], K, 1, nrun, (12,), fut[1:2, 11:12], window_ids=[1], sig_range=sig[1:2],
                                     save_range=save[1:2], sigma_signal=ssg[1:2], kappa=0.5, n_samples=ns)
    assert np.array_equal(alone["sigvals"][0], body[1]) and np.array_equal(alone["mu"][0], out["mu"][1])


@pytest.mark.parametrize("K,L", SIGSMOOTH, ids=["K%d-L%d" % c for c in SIGSMOOTH])
def test_smoothed_and_filtered_means_on_the_signal_path(hmclib, oracle, K, L):
    """extras.pi_smooth_mean / pi_filter_mean together with extras.sig_range (SURVEY 8f rank 2 on the estimatesignals! path):
    the draw average, over all noise samples, of the smoothed (backwardupdate_P!, src/Hmc.jl:442-457) and filtered
    probabilities in sorted labels, against the oracle's literal Pb recursion run on the same noisy data."""
    assert len(SIGSMOOTH) >= 9
    Tmax = 256 * L - (1 if L > 1 else 0)
    lens = [Tmax, max(256 * (L // 2) + 1 if L > 1 else 2, Tmax - 77)]
    Y, Tw, fut = synth.generate_panel(2, Tmax, K, ragged=lens)
    sig = np.stack([Tw - np.array([30, 1]), Tw], axis=1).astype(np.int32)
    ssig = np.array([0.4, 0.9])
    burnin, nrun, ns = 2, 4, 3
    g = _lib.estimate_batch_host(Y, Tw, K, burnin, nrun, (12,), fut[:, 11:12], want_state=True, sig_range=sig, save_range=sig,
                                 sigma_signal=ssig, kappa=0.6, n_samples=ns, alpha=2.0, nu=2.0, want_smooth=True, want_filter_mean=True)
    assert g["steps_per_thread"] == L and g["helper_waves"] == 0
    assert g["occupancy"] == 1                                              # every sigsmooth row is the plain flavour, OCC 1
    for w in range(2):
        T = int(Tw[w])
        o = oracle.estimate_signals(Y[w, :T], K, burnin, nrun, ns, sig=tuple(sig[w]), kappa=0.6, alpha=2.0, nu=2.0,
                                    sigma_signal=float(ssig[w]), save=tuple(sig[w]), yreal=fut[w, 11:12], window_id=w,
                                    want_smooth=True, want_filter_mean=True)
        assert_window_matches_oracle(g, w, T, o, fields=("mu", "pi_smooth_mean", "pi_filter_mean"))
        assert np.max(np.abs(g["pi_smooth_mean"][w, :T].sum(axis=1) - 1)) < 1e-12


@pytest.mark.parametrize("K,T,stream", [(8, 700, False), (5, 300, False), (6, 1100, True), (3, 2600, False), (4, 2400, True), (3, 9000, True)])
def test_smoothed_means_on_the_signal_path_lds_resident_kernel(hmclib, oracle, monkeypatch, K, T, stream):
    """The same for K >= 5 and for longer K <= 4 windows: the smoothing pass of the LDS-resident kernel together with its
    signal path, LDS-resident and HBM-streaming forms (T = 9000 is beyond the LDS by itself).  The last two refusals of the
    hot path (`signal path with smoothed-probability means: K <= 4 only`, smoothing beyond the LDS) are gone."""
    if stream and T < 7000:
        monkeypatch.setenv("HMCG_FORCE_STREAM", "1")
    lens = [T, T - 77]
    Y, Tw, fut = synth.generate_panel(2, T, K, ragged=lens)
    sig = np.stack([Tw - np.array([30, 1]), Tw], axis=1).astype(np.int32)
    ssig = np.array([0.4, 0.9])
    burnin, nrun, ns = 2, 3, 2
    g = _lib.estimate_batch_host(Y, Tw, K, burnin, nrun, (12,), fut[:, 11:12], want_state=True, sig_range=sig, save_range=sig,
                                 sigma_signal=ssig, kappa=0.6, n_samples=ns, alpha=2.0, nu=2.0, want_smooth=True, want_filter_mean=True)
    L = (T + 255) // 256
    assert g["steps_per_thread"] == L and g["helper_waves"] == 0 and g["streaming"] == stream
    for w in range(2):
        Tn = int(Tw[w])
        o = oracle.estimate_signals(Y[w, :Tn], K, burnin, nrun, ns, sig=tuple(sig[w]), kappa=0.6, alpha=2.0, nu=2.0,
                                    sigma_signal=float(ssig[w]), save=tuple(sig[w]), yreal=fut[w, 11:12], window_id=w,
                                    want_smooth=True, want_filter_mean=True)
        assert_window_matches_oracle(g, w, Tn, o, fields=("mu", "fcast", "pi_smooth_mean", "pi_filter_mean"))


@pytest.mark.parametrize("K,T", [(3, 9000), (8, 7000), (2, 12000)])
def test_smoothed_means_beyond_the_lds(hmclib, oracle, K, T):
    """extras.pi_smooth_mean / pi_filter_mean on windows longer than a CU's LDS holds: the smoothing variant of the HBM-streaming form."""
    Y, Tw, fut = synth.generate_panel(1, T, K)
    g = _lib.estimate_batch_host(Y, Tw, K, 1, 3, (12,), fut[:, 11:12], want_state=True, want_smooth=True, want_filter_mean=True)
    o = oracle.estimate_window(Y[0], K, 1, 3, (12,), fut[0, 11:12], window_id=0, want_smooth=True)
    assert g["streaming"]
    assert_window_matches_oracle(g, 0, T, o, fields=("pi_smooth_mean", "mu", "pif_final"))
