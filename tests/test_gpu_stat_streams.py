"""The frame the nine statistic device entries share (stat_device() in csrc/hmcg.hip), on the GPU: work enqueued on a caller's
stream behind the library's earlier work there, returning after the enqueue; context-owned arenas that grow while an earlier
call may still be running and are shared, through one event, with every other statistic and with the sampler's device entry.
The kernels themselves are held to exact references elsewhere (tests/test_stat_coverage.py); here every result must equal, bit
for bit, the same call made alone on the library stream -- the kernels are deterministic -- and pass its feature's reference
check (stat_device_entry.StatCall.check: the *_cases modules, bounds unchanged).

Shapes (stat_device_entry.SHAPES and the settings beside it): K = 3, horizons (0, 12) so that A is read; small = 1 window x 65
draws, large = 3 windows x 2065 draws (three slabs of PRED_SLAB), small2 = small with another seed; a grid of 65 points, PROBS5
and one refinement round, 64 bins with cuts (nd,) and trace (nd // 7, 7), PROBS3, L = the smallest lag of the autocorr table,
score stride 3 (inside score_cases.PAIR_BUDGET, asserted).

(a) late inputs: the device inputs hold NaN; on one caller stream a delay, then asynchronous copies of the real inputs, then the
    untimed call; the stream alone is waited for.  A launch that went to another stream starts at once -- enqueueing ten
    launches takes tens of microseconds --, reads NaN or a stale arena and fails the comparison.
(b) a timed call on a caller's stream reports its launches and a positive time, same bits.
(c) small, large, small2 back to back on two alternating streams from empty arenas (after hmcg_shutdown): call 2 grows the
    arena while call 1 may still be running, call 3 returns to the small shape in the grown arena.  Runs once.
(d) all nine on one set of draws with the sampler's device entry (K = 8, LDS-resident, extras.corr: both users of the shared
    event) in between, alternating over two streams, one sync.
(e) the pipeline a caller writes: a delay, DevicePanel.run(stream=s) and the nine panel statistics with no host wait between
    them; each equals the entry run alone afterwards on the panel's fetched draws.

The delay is a chain of COPIES device-to-device copies of a DELAY_BYTES tensor on the stream, bracketed by torch events; every
test that uses it asserts that it lasted at least DELAY_FLOOR_MS = 5 ms, a condition on the test, not a measurement of the code:
about a hundred times what a misdirected kernel needs to start early.  On an MI355X COPIES = 64 copies of 512 MiB measured
14.4 and 14.3 ms alone (16 copies 3.6 ms, 128 copies 28.8 ms: 0.225 ms a copy) and 12.8 to 14.5 ms over the module's ten
uses in (a) and (e): more than twice the floor.  The module's wall time there: 4.0 s for its 30 tests, the slowest 0.5 s ((e))
and 0.4 s ((a) of the scores); the stand-alone runs and the references are made once and shared."""
import numpy as np
import pytest

import autocorr_cases as ac
import device_entry as de
import score_cases as sc
import stat_device_entry as sde

pytestmark = pytest.mark.gpu

FEATURES = tuple(sde.FEATURES)
DELAY_BYTES = 512 << 20
COPIES = 64
DELAY_FLOOR_MS = 5.0
_cases, _alone = {}, {}


def case_of(feature, shape):
    """The feature's case on a shape of sde.SHAPES, made once: its reference is computed once and kept in it."""
    if (feature, shape) not in _cases:
        _cases[feature, shape] = sde.stream_case(feature, shape)
    return _cases[feature, shape]


def alone(feature, shape):
    """The stand-alone timed run of that case on the library stream (launches and kernel time asserted there), made once."""
    if (feature, shape) not in _alone:
        _alone[feature, shape] = sde.run(feature, case_of(feature, shape), timed=True)
    return _alone[feature, shape]


class Delay:
    """COPIES copies of one large tensor to and fro on a stream, between two timed events of that stream."""

    def __init__(self):
        import torch
        self.torch = torch
        self.a = torch.zeros(DELAY_BYTES // 8, dtype=torch.float64, device="cuda:0")
        self.b = torch.zeros_like(self.a)
        self.ev = None

    def enqueue(self, stream):
        torch = self.torch
        self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        with torch.cuda.stream(stream):
            self.ev[0].record(stream)
            for i in range(COPIES):
                (self.b if i % 2 == 0 else self.a).copy_(self.a if i % 2 == 0 else self.b, non_blocking=True)
            self.ev[1].record(stream)

    def check(self):
        """After the stream has been waited for: the delay was long enough for the test to mean something."""
        ms = self.ev[0].elapsed_time(self.ev[1])
        print("delay: %d copies of %d MiB took %.2f ms" % (COPIES, DELAY_BYTES >> 20, ms))
        assert ms >= DELAY_FLOOR_MS, ms


@pytest.fixture(scope="module")
def delay():
    d = Delay()
    d.torch.cuda.synchronize()
    yield d
    del d.a, d.b


def test_settings_are_the_ones_chosen():
    from hmc_jl_amd import _lib
    import test_gpu_autocorr as ta
    assert _lib.PRED_SLAB == 1024 and sde.SHAPES["large"][1] > 2 * _lib.PRED_SLAB
    assert case_of("chain_autocorr", "small")["L"] == min(c[1] for c in ta._cases()) == min(ac.LAG_EDGES)
    W, nd, _ = sde.SHAPES["large"]
    stride, n_u = sc.thinning(nd, case_of("predictive_scores", "large")["stride"])
    assert sc.pair_cost(sde.K, n_u, W) <= sc.PAIR_BUDGET


@pytest.mark.parametrize("feature", FEATURES)
def test_late_inputs_on_the_callers_stream(feature, delay):
    import torch
    c = sde.prepare(feature, case_of(feature, "large"))
    c.poison_inputs()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    delay.enqueue(s)
    c.fill_inputs_on(s)
    assert c.enqueue(s, timed=False) is None
    s.synchronize()                                          # the caller's stream alone
    delay.check()
    got = c.collect()
    sde.assert_same_bits(got, alone(feature, "large"), "%s behind late inputs on a caller's stream" % feature)
    c.check(got, "%s, late inputs" % feature)


@pytest.mark.parametrize("feature", FEATURES)
def test_timed_call_on_the_callers_stream(feature):
    import torch
    c = sde.prepare(feature, case_of(feature, "large"))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    tm = c.enqueue(s, timed=True)
    assert tm.kernel_ms > 0.0 and tm.launches == c.f.launches(c.case), (tm.kernel_ms, tm.launches)
    sde.assert_same_bits(c.collect(), alone(feature, "large"), "%s timed on a caller's stream" % feature)


@pytest.mark.parametrize("feature", FEATURES)
def test_back_to_back_across_two_streams_with_growth(feature):
    """Modelled on test_gpu_device_entry.test_shared_scratch_across_calls_and_streams."""
    import torch
    from hmc_jl_amd import _lib
    shapes = ("small", "large", "small2")
    calls = [sde.prepare(feature, case_of(feature, sh)) for sh in shapes]          # uploads, allocations, prefills: before the first enqueue
    torch.cuda.synchronize()
    _lib.load().hmcg_shutdown()                              # a new context: the arenas start empty, so call 2 grows one
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for i, c in enumerate(calls):                            # nothing between the enqueues: each may find the previous one running
        c.enqueue(streams[i % 2], timed=False)
    torch.cuda.synchronize()
    got = [c.collect() for c in calls]
    for sh, c, g in zip(shapes, calls, got):
        sde.assert_same_bits(g, alone(feature, sh), "%s, %s of small / large / small2 back to back" % (feature, sh))
        c.check(g, "%s, %s back to back" % (feature, sh))


def test_all_features_interleaved_with_the_sampler():
    import torch
    from hmc_jl_amd import synth
    W, nd, seed = sde.SHAPES["large"]
    draws = sde.panel_draws(seed + 100, W, nd)
    cases = {f: sde.stream_case(f, draws=draws, nd=nd) for f in FEATURES}
    Y, Tw, fut = synth.generate_panel(2, 300, 8)
    args, kw = (Y, Tw, 8, 1, 3, (12,), fut[:, 11:12]), dict(want_corr=True)
    queue = [sde.prepare(f, cases[f]) for f in FEATURES]
    queue.insert(4, de.prepare_call(*args, **kw))           # the sampler's device entry: the LDS-resident kernel's scratch and extras.corr
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for i, c in enumerate(queue):
        c.enqueue(streams[i % 2], timed=False)
    torch.cuda.synchronize()
    got = [c.collect() for c in queue]
    sampler = got.pop(4)
    for f, g in zip(FEATURES, got):
        sde.assert_same_bits(g, sde.run(f, cases[f]), "%s among all nine and the sampler" % f)
    single = de.estimate_batch_device_np(*args, **kw)
    assert (single["status"] == 0).all() and "corr" in de.arrays_of(single)
    for k, v in de.arrays_of(single).items():
        assert np.array_equal(sampler[k], v, equal_nan=True), ("sampler", k)


def panel_blocks(feature, out):
    """A DevicePanel statistic's tensors as the output blocks of the feature's row, in its order."""
    order = {"chain_density": ("range", "counts", "stats", "trace"), "chain_autocorr": ("acov", "diag"), "chain_quantiles": ("q", "n"),
             "ergodic_moments": ("cols", "out", "n"), "predictive_quantiles": ("out", "range", "flag")}
    tensors = [out[k] for k in order[feature]] if feature in order else [out]
    return [t.cpu().numpy() for t in tensors]


def test_panel_pipeline_on_one_caller_stream(delay):
    """run(stream=s) and every statistic of the panel behind it with no host wait in between: the statistics follow the run
    onto its stream, so none reads the draws before the sweep has written them."""
    import torch
    from hmc_jl_amd import _lib, synth
    from hmc_jl_amd.device import DevicePanel
    Kp, T, W, nrun = sde.K, 200, 2, sde.SHAPES["large"][1]
    Y, Tw, fut = synth.generate_panel(W, T, Kp)
    p = DevicePanel(Y, Tw, Kp, nrun, (12,), fut[:, 11:12])
    yreal = np.random.default_rng(5).normal(2.0, 3.0, size=(len(sde.HORIZONS), W))
    s = torch.cuda.Stream()
    delay.enqueue(s)
    assert p.run(burnin=20, timed=False, stream=s.cuda_stream) is None
    L = min(ac.LAG_EDGES)
    out = {"predictive_cdf": p.predictive_cdf(sde.pc.make_grid(sde.GRID), sde.HORIZONS),
           "bias_moments": p.bias_moments(max(sde.HORIZONS)),
           "mixture_moments": p.mixture_moments(sde.HORIZONS),
           "chain_density": p.chain_density("mu", (nrun,), sde.BINS, None, (nrun // 7, 7)),
           "chain_autocorr": p.chain_autocorr("mu", L),
           "chain_quantiles": p.chain_quantiles("mu", sde.qc.PROBS3),
           "ergodic_moments": p.ergodic(cols=True),
           "predictive_quantiles": p.fan(sde.fc.PROBS5, sde.HORIZONS, sde.ROUNDS),
           "predictive_scores": p.scores(sde.HORIZONS, yreal, sde.SCORE_STRIDE)}
    p.sync()
    delay.check()
    assert (p.status.cpu().numpy() == 0).all()
    d = {n: getattr(p, n).cpu().numpy() for n in _lib.DRAW_KEYS}
    draws = dict(mu=d["mu"], sig2=d["sig2"], pi=d["pi_end"], A=d["A"], fcast=d["fcast"], yreal=yreal)
    assert all(np.abs(d[n]).max() > 0.0 for n in _lib.DRAW_KEYS)
    cases = {f: sde.stream_case(f, draws=draws, nd=nrun) for f in FEATURES}         # the settings above are those of stream_case
    got = {f: sde.FEATURES[f].unpack(cases[f], panel_blocks(f, out[f])) for f in FEATURES}
    wrong = ["%s (%s)" % (f, ", ".join(bad)) for f in FEATURES for bad in [sde.differing_fields(got[f], sde.run(f, cases[f]))] if bad]
    assert not wrong, "panel statistics differ from the entries run alone on the fetched draws: " + "; ".join(wrong)
    for f in FEATURES:
        row = sde.FEATURES[f]
        row.check(cases[f], got[f], row.reference(cases[f]), "panel %s" % f)
