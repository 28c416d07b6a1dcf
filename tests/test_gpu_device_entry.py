"""hmcg_estimate_batch_device -- the entry bench.py times -- on every kernel family, every extras pointer and RESUME.

The rest of the GPU suite reaches launch_device (csrc/hmcg.hip) through DevicePanel alone: the K = 3 base path plus extras.corr.
Here the device entry is driven by tests/device_entry.py, a runner with the host runner's interface over torch-allocated HBM
buffers that are prefilled with a sentinel (NaN / 0x5a bytes), so that what a kernel leaves unwritten, or reads before it
writes, shows.
  (a) PARITY_CASES: oracle parity through the device entry with the very assertions of the host-entry cases (states bit-exact,
      floats within TOL = 1e-9 relative to 1 + |x|, status the oracle's), one case per kernel family and extras path; the same
      call through the host entry agrees bit for bit wherever the host selects the same plan (ragged register-resident batches:
      with the min_T hint); the timing record proves which kernel ran.
  (b) SPLIT_CASES: a chain cut with sweep_count / HMCG_FLAG_RESUME into launches that carry status, xstate, sumacc,
      sample_summary and the running smoothed / filtered sums in the same device buffers and write their draws into the same
      full-length arrays equals the one-launch chain bit for bit -- cuts inside burn-in, exactly at burnin, after kept draws,
      inside a noise sample and at a sample boundary, on the register-resident kernel (every flavour), the LDS-resident base, SIG,
      SM and SIG + SM forms and the streaming form.
  (c) the entry's contract: a call without RESUME does not depend on what its buffers hold; skipped windows are flagged and
      every byte of their outputs is left alone; smoothing on the LDS-resident kernel without extras.pif_final is refused with
      nothing written; work enqueued on the caller's stream is complete once that stream is; calls that share the context's
      scratch arena across two streams, while it grows, each equal their stand-alone run.
Every comparison between two GPU runs is exact; no new tolerance.  tests/test_variant_coverage.py (no GPU) holds the tables below
to include/hmcg.h: every pointer member of hmcg_extras is passed by some case, every kernel form is split."""
import numpy as np
import pytest

import device_entry as de
from hmc_jl_amd import _lib, synth
from device_entry import arrays_of, assert_device_equals_host, kept_after
from kernel_tables import FLAVOUR_WAVES, NT, STREAM_T, coverage_lengths, ladder_ceiling, register_classes
from oracle_parity import (SIGMA_SIGNAL, assert_ran_on_big, assert_same, check_against_oracle, check_signals_against_oracle,
                           check_smoothing_against_oracle, check_tail_signals_against_oracle, check_teacher_forced_against_oracle,
                           signal_ranges)

pytestmark = pytest.mark.gpu

# the hmcg_extras pointer members every call of a path passes on the device entry; call_of holds each case to what the runner
# really puts into the struct for it (device_entry.extras_passed)
STATE = ("x_final", "pif_final", "xstate", "sumacc")
SIGNAL = ("sig_range", "save_range", "sigvals", "sigma_signal", "sample_summary")
SMOOTH = ("pi_smooth_mean", "pi_filter_mean", "pi_smooth_draws")
PATH_EXTRAS = {
    "base": STATE,
    "teacher": STATE + ("x_init",),
    "sig": STATE + SIGNAL,
    "tail": STATE + SIGNAL + ("end_pos",),
    "smooth": STATE + SMOOTH,
    "sig+smooth": STATE + SIGNAL + SMOOTH,
}
EXTRA_MEMBER = {"window_ids": "window_ids", "want_corr": "corr"}          # a case's extra keyword -> the member it adds


def case(id, kernel, path, K, lens, sweeps, bucketed=None, extra=(), **opt):
    """kernel: register | lds | stream (what the production dispatch must pick).  sweeps: (burnin, nrun).  bucketed: the min_T
    hint is passed (default: whenever a register-resident batch is ragged -- the host entry then runs the same plan)."""
    if bucketed is None:
        bucketed = kernel == "register" and len(set(lens)) > 1
    return dict(id=id, kernel=kernel, path=path, K=K, lens=list(lens), sweeps=sweeps, bucketed=bucketed, extra=tuple(extra), **opt)


def tail_lens(T):
    return [T, T - 7, T - 64]


PARITY_CASES = [
    # register-resident base: three steps-per-thread classes in one batch, one launch sized for the longest / bucketed
    case("reg-base-K2", "register", "base", 2, [513, 257, 64, 2], (2, 4), bucketed=False),
    case("reg-base-K2-bucketed", "register", "base", 2, [513, 257, 64, 2], (2, 4), bucketed=True, extra=("want_corr",)),
    case("reg-base-K4", "register", "base", 4, [513, 257, 64, 2], (2, 4), bucketed=False),
    case("reg-base-K4-bucketed", "register", "base", 4, [513, 257, 64, 2], (2, 4), bucketed=True, extra=("window_ids",)),
    # LDS-resident base: K = 3 beyond the register ladder; K = 5; K = 8 (two output passes)
    case("lds-base-K3", "lds", "base", 3, coverage_lengths(False, False, False, 3), (2, 4)),
    case("lds-base-K5", "lds", "base", 5, coverage_lengths(False, False, False, 5), (2, 4)),
    case("lds-base-K8", "lds", "base", 8, coverage_lengths(False, False, False, 8), (2, 4)),
    # streaming base: 1 + 2 sweeps (the oracle's cost is set here)
    case("stream-base-K3", "stream", "base", 3, coverage_lengths(False, False, True, 3), (1, 2)),
    case("stream-base-K8", "stream", "base", 8, coverage_lengths(False, False, True, 8), (1, 2)),
    # signal path: sigvals, save_range, sample_summary, three chained noise samples
    case("reg-sig-K3", "register", "sig", 3, [400, 400, 400], (2, 3)),
    case("lds-sig-K6", "lds", "sig", 6, [300, 297, 150], (2, 3)),
    # signals past the end date: end_pos, blend_mask = 1, horizons (0, 12)
    case("reg-tail-K3", "register", "tail", 3, tail_lens(300), (2, 4), sigLen=12),
    case("lds-tail-K8", "lds", "tail", 8, tail_lens(400), (2, 4), sigLen=48),
    # smoothing: pi_smooth_mean, pi_filter_mean, pi_smooth_draws
    case("reg-smooth-K3", "register", "smooth", 3, [1000, 257, 64], (2, 4)),
    case("lds-smooth-K5", "lds", "smooth", 5, [600, 65], (2, 4)),
    case("stream-smooth-K3", "stream", "smooth", 3, coverage_lengths(False, True, True, 3), (1, 2)),
    # teacher forcing: x_init with random states, x_final and pif_final after one sweep
    case("reg-teacher-K4", "register", "teacher", 4, [700, 700, 700], (0, 1)),
    case("lds-teacher-K7", "lds", "teacher", 7, [300, 300, 300], (0, 1)),
]
N_SAMPLES = 3


def case_extras(c):
    """The hmcg_extras pointer members the case's call passes."""
    return set(PATH_EXTRAS[c["path"]]) | {EXTRA_MEMBER[k] for k in c["extra"]}


def call_of(c):
    """(args, kw) of the case's call, for either entry: what the oracle checkers pass for it (held to that by Recorder)."""
    K, lens, path = c["K"], c["lens"], c["path"]
    W = len(lens)
    Y, Tw, fut = synth.generate_panel(W, max(lens), K, ragged=lens)
    burnin, nrun = c["sweeps"]
    horizons, yreal = (12,), fut[:, 11:12]
    kw = dict(want_state=True)
    sig_kw = dict(kappa=0.6, n_samples=N_SAMPLES, alpha=2.0, nu=2.0, want_sample_summary=True)
    if path == "teacher":
        horizons, yreal = (), None
        kw["x_init"] = np.random.default_rng(11 + K).integers(0, K, size=Y.shape).astype(np.int32)
    elif path in ("sig", "sig+smooth"):
        sig, save = signal_ranges(Tw)
        if path == "sig+smooth":
            save = sig                                       # (as check_smoothing_against_oracle reports the signal values)
        kw.update(sig_range=sig, save_range=save, sigma_signal=SIGMA_SIGNAL[:W], **sig_kw)
    elif path == "tail":
        n = c["sigLen"]
        sig = np.stack([Tw - n, Tw], axis=1).astype(np.int32)
        horizons, yreal = (0, 12), np.stack([fut[:, 0], fut[:, 11]], axis=1)     # slot 0 is the blend (h == sigLen), slot 1 is h = sigLen + 12
        kw.update(sig_range=sig, save_range=sig, sigma_signal=np.array([0.4, 1.3, 0.05]), end_pos=(Tw - 1 - n).astype(np.int32),
                  blend_mask=1, **sig_kw)
    if path in ("smooth", "sig+smooth"):
        kw.update(want_smooth=True, want_filter_mean=True, want_smooth_draws=True)
    if "window_ids" in c["extra"]:
        kw["window_ids"] = np.array([7, 3, 11, 5][:W])
    if "want_corr" in c["extra"]:
        kw["want_corr"] = True
    args = (Y, Tw, K, burnin, nrun, horizons, yreal)
    passed = de.extras_passed(*args, **kw, **device_kw(c))
    assert passed == case_extras(c), (c["id"], sorted(passed ^ case_extras(c)))
    return args, kw


def device_kw(c):
    """The device entry's own keywords of the case: the min_T hint."""
    valid = [t for t in c["lens"] if t >= 2]
    return dict(min_T=min(valid)) if c["bucketed"] else {}


class Recorder:
    """The device runner as the `run=` of an oracle checker; holds the checker's call to the case's table entry."""

    def __init__(self, c):
        self.c = c
        self.args, self.kw = call_of(c)

    def __call__(self, *a, **kw):
        for x, y in zip(a, self.args):
            assert (x is None and y is None) or np.array_equal(np.asarray(x), np.asarray(y))
        assert kw.get("seed", 1234) == 1234
        on = {k: v for k, v in kw.items() if v is not None and v is not False and k != "seed"}
        mine = {k: v for k, v in self.kw.items() if v is not None and v is not False}
        assert sorted(on) == sorted(mine), (sorted(on), sorted(mine))
        for k in on:
            assert np.array_equal(np.asarray(on[k]), np.asarray(mine[k])), k
        return de.estimate_batch_device_np(*self.args, **self.kw, **device_kw(self.c))


# ---- which kernel ran ----
def assert_ran_as_planned(g, c):
    path, K, lens = c["path"], c["K"], c["lens"]
    sig, smooth = path in ("sig", "tail", "sig+smooth"), path in ("smooth", "sig+smooth")
    maxT = max(lens)
    if c["kernel"] == "register":
        Ls = register_classes(K, sig, smooth)
        hi = next(i for i, L in enumerate(Ls) if NT * L >= maxT)
        lo = next(i for i, L in enumerate(Ls) if NT * L >= min(t for t in lens if t >= 2)) if c["bucketed"] else hi
        assert g["occupancy"] in (1, 2) and not g["streaming"], (g["occupancy"], g["streaming"])
        assert g["threads_per_window"] == NT and g["steps_per_thread"] == Ls[hi], (g["steps_per_thread"], Ls[hi])
        assert g["buckets"] == hi - lo + 1, (g["buckets"], hi - lo + 1)      # the device entry launches every class between the two
        if not c["bucketed"]:
            assert g["buckets"] == 1
    else:
        assert maxT > ladder_ceiling(K, sig, smooth)                          # the production route, no HMCG_FORCE_BIG
        assert_ran_on_big(g, c["kernel"] == "stream", maxT, sig, smooth)


# ---- (a) oracle parity through the device entry; the host entry agrees bit for bit ----
@pytest.mark.parametrize("c", PARITY_CASES, ids=[c["id"] for c in PARITY_CASES])
def test_device_entry_against_oracle(hmclib, oracle, c):
    run = Recorder(c)
    (Y, Tw, K, burnin, nrun, horizons, yreal), kw = run.args, run.kw
    path = c["path"]
    if path == "base":
        g = check_against_oracle(oracle, Y, Tw, K, burnin, nrun, horizons, yreal, window_ids=kw.get("window_ids"), run=run,
                                 **{k: kw[k] for k in ("want_corr",) if k in kw})
    elif path == "sig":
        g = check_signals_against_oracle(oracle, Y, Tw, K, burnin, nrun, N_SAMPLES, kw["sig_range"], kw["save_range"], 0.6, 2.0, 2.0,
                                         kw["sigma_signal"], yreal, run=run)
    elif path == "tail":
        g = check_tail_signals_against_oracle(oracle, Y, Tw, K, burnin, nrun, N_SAMPLES, kw["sig_range"], kw["save_range"], kw["sigma_signal"],
                                              kw["end_pos"], horizons, yreal, c["sigLen"], want_sample_summary=True, run=run)
    elif path == "smooth":
        g = check_smoothing_against_oracle(oracle, Y, Tw, K, burnin, nrun, yreal, run=run, want_smooth_draws=True)
        for w, T in enumerate(Tw):                           # (the checker held the per-draw array to the oracle's pib at TOL)
            draws = g["pi_smooth_draws"][w, :, :T, :]        # (K, T, nd)
            assert np.max(np.abs(draws.mean(axis=2).T - g["pi_smooth_mean"][w, :T])) < 1e-12
            assert np.max(np.abs(draws[:, -1, :] - g["pi_end"][w])) < 1e-12      # pib[:, end, :] is what pi_end reports
    else:
        g = check_teacher_forced_against_oracle(oracle, Y, Tw, K, kw["x_init"], run=run)
        assert (g["status"] == 0).all()
    assert_ran_as_planned(g, c)
    if c["kernel"] == "register" and len(set(c["lens"])) > 1 and not c["bucketed"]:
        return                                               # one launch sized for the longest window: not the host entry's plan
    h = _lib.estimate_batch_host(*run.args, **kw)
    assert (h["steps_per_thread"], h["streaming"], h["occupancy"] > 0) == (g["steps_per_thread"], g["streaming"], g["occupancy"] > 0)
    assert_device_equals_host(g, h, Tw, kw.get("save_range"))


# ---- (c) a call without RESUME does not depend on what its buffers hold ----
@pytest.mark.parametrize("c", PARITY_CASES, ids=[c["id"] for c in PARITY_CASES])
def test_fresh_call_ignores_buffer_contents(hmclib, c):
    """The same call three times into the same device buffers: over the sentinel (status over 0x5a5a5a5a garbage), over its own
    results, and once more enqueue-only followed by a device sync.  Every output must equal the first run's: a kernel that adds
    into a caller's buffer (the running smoothed / filtered sums, the per-sample summaries) without starting it shows here."""
    args, kw = call_of(c)
    first = de.estimate_batch_device_np(*args, **kw, **device_kw(c))
    assert (first["status"] == 0).all(), first["status"]
    again = de.estimate_batch_device_np(*args, **kw, **device_kw(c), out=first)
    assert again["_call"].buf is first["_call"].buf
    assert_same(again, first, what="second run into dirty buffers")
    third = de.estimate_batch_device_np(*args, **kw, **device_kw(c), out=first, timed=False)
    assert third["kernel_ms"] is None
    assert_same(third, first, what="third run, enqueue-only")


# ---- (b) split chains ----
BASE_SWEEPS, BASE_SPLITS = (3, 5), ((1,), (3,), (5,), (2, 5))             # cut after these sweeps: in burn-in, at burnin, kept; three pieces
SIG_SWEEPS, SIG_SPLITS = (2, 4), ((1,), (4,), (6,), (9,))                 # in sample 0 before / after its first kept draw, boundary, mid-sample 1


def split(id, form, kernel, path, K, T, env=()):
    """form: what the coverage contract counts (register, lds, streaming, sig, sm, sig+sm)."""
    sig = path in ("sig", "sig+smooth")
    return dict(id=id, form=form, kernel=kernel, path=path, K=K, lens=[T, T - 37], sweeps=SIG_SWEEPS if sig else BASE_SWEEPS,
                splits=SIG_SPLITS if sig else BASE_SPLITS, env=tuple(env), bucketed=False, extra=())


SPLIT_CASES = [
    split("reg-K2-p1", "register", "register", "base", 2, 300, env=(("HMCG_FLAVOUR", "p1"),)),
    split("reg-K2-p2", "register", "register", "base", 2, 300, env=(("HMCG_FLAVOUR", "p2"),)),
    split("reg-K2-h", "register", "register", "base", 2, 300, env=(("HMCG_FLAVOUR", "h"),)),
    split("reg-K4", "register", "register", "base", 4, 700),
    split("lds-K7", "lds", "lds", "base", 7, 600),
    split("stream-K3-forced", "streaming", "stream", "base", 3, 1500, env=(("HMCG_FORCE_BIG", "1"), ("HMCG_FORCE_STREAM", "1"))),
    split("lds-sig-K5", "sig", "lds", "sig", 5, 300),
    split("lds-sm-K6", "sm", "lds", "smooth", 6, 400),
    split("lds-sigsm-K8", "sig+sm", "lds", "sig+smooth", 8, 300),
]


@pytest.mark.parametrize("c", SPLIT_CASES, ids=[c["id"] for c in SPLIT_CASES])
def test_split_chain_equals_one_launch(hmclib, monkeypatch, c):
    for k, v in c["env"]:
        monkeypatch.setenv(k, v)
    args, kw = call_of(c)
    burnin, nrun = c["sweeps"]
    n_samples = kw.get("n_samples", 1)
    total = n_samples * (burnin + nrun)
    one = de.estimate_batch_device_np(*args, **kw)
    assert (one["status"] == 0).all()
    # the kernel the case is about
    sig, smooth = "sig_range" in kw, "want_smooth" in kw
    if c["kernel"] == "register":
        assert one["occupancy"] in (1, 2) and one["buckets"] == 1 and not one["streaming"]
        for k, v in c["env"]:
            if k == "HMCG_FLAVOUR":
                assert (one["helper_waves"], one["occupancy"]) == FLAVOUR_WAVES[v]
    else:
        assert_ran_on_big(one, c["kernel"] == "stream", max(c["lens"]), sig, smooth)
    draws = [k for k in de.DRAW_KEYS + ("pi_smooth_draws",) if k in one]
    for cuts in c["splits"]:
        ends = list(cuts) + [total]
        g, base = None, 0
        for i, end in enumerate(ends):
            g = de.estimate_batch_device_np(*args, **kw, sweep_base=base, sweep_count=end - base, resume_state=g)
            assert g["launches"] == 1 and (g["status"] == 0).all()
            d = kept_after(end, burnin, nrun, n_samples)
            for k in draws:
                # draws [0, d) stand as the one-launch chain wrote them -- an earlier piece's included --, the rest is untouched
                assert np.array_equal(g[k][..., :d], one[k][..., :d], equal_nan=True), (cuts, i, k)
                assert np.isnan(g[k][..., d:]).all(), (cuts, i, k, "a draw beyond this piece was written")
            base = end
        assert_same(g, one, what="pieces %s" % (cuts,))


# ---- (c) skipped windows ----
SKIP_CASES = [("register", 3, "base"), ("bucketed", 3, "base"), ("lds", 5, "base"), ("register", 3, "sig"), ("lds", 5, "sig")]


@pytest.mark.parametrize("kernel,K,path", SKIP_CASES, ids=["%s-K%d-%s" % s for s in SKIP_CASES])
def test_skipped_windows_are_left_untouched(hmclib, kernel, K, path):
    """include/hmcg.h: the device entry flags a skipped window in status and leaves its outputs alone.  One NaN observation, one
    T = 1, one T beyond what max_T was sized for and, on the signal path, one bad sig_range, between good windows; every byte of
    every output of the skipped ones is still the sentinel, the good ones equal their single-window calls."""
    max_T, ldY = 300, 2 * NT + 8                             # max_T sizes two steps per thread: T = ldY is beyond them
    good = [300, 130, 257]
    Y = np.zeros((7, ldY))
    Yg, _, fut = synth.generate_panel(7, max_T, K)
    Y[:, :max_T] = Yg
    Tw = np.array([good[0], 200, good[1], 1, ldY, good[2], 280], dtype=np.int32)
    Y[4, max_T:] = Y[4, :ldY - max_T]
    Y[1, 10] = np.nan
    want = np.array([0, _lib.ST_NONFINITE, 0, _lib.ST_BAD_T, _lib.ST_BAD_T, 0, 0], dtype=np.int32)
    kw = dict(want_state=True)
    if path == "sig":
        sig = np.stack([Tw - 12, Tw], axis=1).astype(np.int32)
        sig[3] = (0, 1)
        sig[6] = (Tw[6] - 10, Tw[6] - 3)                     # a non-empty range that does not end at T
        want[6] = _lib.ST_BAD_RANGE
        kw.update(sig_range=sig, save_range=np.stack([np.maximum(Tw - 3, 0), Tw], axis=1).astype(np.int32),
                  sigma_signal=np.linspace(0.2, 0.8, 7), kappa=0.6, n_samples=2, alpha=2.0, nu=2.0, want_sample_summary=True)
    dev = dict(max_T=max_T, min_T=min(good)) if kernel == "bucketed" else dict(max_T=max_T)
    g = de.estimate_batch_device_np(Y, Tw, K, 1, 3, (12,), fut[:, 11:12], **kw, **dev)
    assert np.array_equal(g["status"], want), g["status"]
    if kernel == "lds":
        assert g["occupancy"] == 0 and g["steps_per_thread"] == 2 and g["buckets"] == 1
    else:
        assert g["occupancy"] in (1, 2) and g["steps_per_thread"] == 2 and g["buckets"] == (2 if kernel == "bucketed" else 1)
    outputs = [k for k in arrays_of(g) if k != "status"]
    for w in np.nonzero(want)[0]:
        for k in outputs:
            assert np.array_equal(g[k][w], de.sentinel_like(g[k][w]), equal_nan=True), (w, k, "a skipped window's output was written")
    for w in np.nonzero(want == 0)[0]:
        # alone: the same launch shape (one launch: sized by the call's max_T; bucketed: by the window's own length)
        one_kw = {k: (v[w:w + 1] if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        s = de.estimate_batch_device_np(Y[w:w + 1], Tw[w:w + 1], K, 1, 3, (12,), fut[w:w + 1, 11:12], window_ids=np.array([w]), **one_kw,
                                        max_T=int(Tw[w]) if kernel == "bucketed" else max_T)
        assert s["status"][0] == 0
        for k in outputs:
            assert np.array_equal(g[k][w], s[k][0], equal_nan=True), (w, k)


# ---- (c) the needs_pif refusal ----
def test_lds_resident_smoothing_without_pif_final_is_refused(hmclib):
    K, lens = 5, [600, 65]
    Y, Tw, fut = synth.generate_panel(len(lens), max(lens), K, ragged=lens)
    args = (Y, Tw, K, 1, 3, (12,), fut[:, 11:12])
    kw = dict(want_smooth=True, want_filter_mean=True)
    ok = de.estimate_batch_device_np(*args, **kw)
    assert (ok["status"] == 0).all() and ok["occupancy"] == 0
    with pytest.raises(_lib.HmcgError, match="pif_final") as e:
        de.estimate_batch_device_np(*args, **kw, pass_pif=False)
    assert "rc=-1:" in str(e.value)                          # HMCG_E_BADARG
    e.value.call.torch.cuda.synchronize()
    left = e.value.call.collect()
    assert "pif_final" not in left
    for k, v in arrays_of(left).items():
        assert np.array_equal(v, de.sentinel_like(v), equal_nan=True), (k, "written by a refused call")
    assert_same(de.estimate_batch_device_np(*args, **kw), ok, what="the next valid call")
    # the register-resident smoothing kernels keep pif in registers: no pif_final needed
    Y3, T3, f3 = synth.generate_panel(2, 300, 3)
    r = de.estimate_batch_device_np(Y3, T3, 3, 1, 3, (12,), f3[:, 11:12], **kw, pass_pif=False)
    assert (r["status"] == 0).all() and r["occupancy"] in (1, 2) and np.isfinite(r["pi_smooth_mean"]).all()


# ---- (c) the caller's stream ----
def test_results_are_complete_once_the_callers_stream_is(hmclib):
    import torch
    lens = [700, 300]
    Y, Tw, fut = synth.generate_panel(len(lens), max(lens), 3, ragged=lens)
    args, kw = (Y, Tw, 3, 2, 6, (12,), fut[:, 11:12]), dict(want_state=True, min_T=300)
    ref = de.estimate_batch_device_np(*args, **kw)                          # the library's own stream, timed
    assert ref["buckets"] > 1                                               # (the bucket streams join the caller's stream)
    s = torch.cuda.Stream()
    g = de.estimate_batch_device_np(*args, **kw, stream=s, timed=False)     # the runner waits for s alone
    assert_same(g, ref, what="caller's stream")


# ---- (c) the context's scratch arena across calls and streams ----
def test_shared_scratch_across_calls_and_streams(hmclib):
    """launch_device carves the pdf scratch and the streaming slabs from one arena of the device context and orders every user
    behind the last one's event (ev_scr); growing waits for that event first.  Four enqueue-only calls back to back on two
    alternating caller streams -- K = 8 / T = 300, K = 8 / T = 1500 (the arena grows), K = 3 / STREAM_T (slabs added), K = 8 /
    T = 300 again --, one sync, and each result equals its stand-alone run.  The sequence runs once."""
    import torch
    shapes = [(8, 300, (1, 3)), (8, 1500, (1, 3)), (3, STREAM_T, (1, 2)), (8, 300, (1, 3))]
    calls = []
    for i, (K, T, (burnin, nrun)) in enumerate(shapes):
        Y, Tw, fut = synth.generate_panel(2, T, K, window_base=10 * i)
        calls.append(((Y, Tw, K, burnin, nrun, (12,), fut[:, 11:12]), dict(want_state=True, window_base=10 * i)))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    pending = [de.prepare_call(*a, **kw) for a, kw in calls]            # uploads, allocations, prefills: all before the first enqueue
    torch.cuda.synchronize()
    _lib.load().hmcg_shutdown()                              # a new context: the arena starts empty, so calls 2 and 3 grow it
    for i, p in enumerate(pending):                          # nothing between the four enqueues: each may find the previous one running
        p.enqueue(streams[i % 2], timed=False)
    torch.cuda.synchronize()
    got = [p.collect() for p in pending]
    for i, ((a, kw), g) in enumerate(zip(calls, got)):
        alone = de.estimate_batch_device_np(*a, **kw)
        assert (alone["status"] == 0).all() and alone["occupancy"] == 0 and alone["streaming"] == (i == 2)
        for k, v in arrays_of(alone).items():
            assert np.array_equal(g[k], v, equal_nan=True), (i, k)
