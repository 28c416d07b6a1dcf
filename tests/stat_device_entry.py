"""The nine hmcg_*_device entries of the draw statistics behind one interface: every input a host array and a torch tensor in
HBM, every output a torch tensor with a sentinel window before and after its block, the library call alone in enqueue().  A
plain module for the GPU tests of the nine features (tests/test_gpu_<feature>.py) and of the frame they share
(tests/test_gpu_stat_streams.py: caller streams, back-to-back enqueues, arena growth); importing it needs neither torch nor a
GPU.  tests/test_stat_stream_cases.py holds FEATURES to the library's exports and to the launch counts of csrc/hmcg.hip.

FEATURES has one row per entry: the _lib call, how a case (a dict of the arguments the feature's tests always passed) becomes
the call's struct, input pointers and output blocks, the *_cases module whose reference and bound judge the result, and the
launches a timed call reports.  prepare() uploads and allocates; StatCall.enqueue() is the library call and nothing else, so
several prepared calls can be enqueued back to back, on any stream, with nothing between them; collect() checks the sentinel
frames and unpacks; check() is the feature's reference comparison.  run() is the stand-alone call the nine modules make.

What the device entries leave to their caller is made visible here:
  * an output is allocated with one more window in front and one behind, all prefilled with a sentinel (SENTINEL in the float
    blocks, ISENTINEL in the integer ones): a write outside [W][...] shows, and so does an output the call was not given;
  * the inputs exist twice, as (pinned) host arrays and as device tensors, so a test can poison the device copies and have the
    real values arrive late, by asynchronous copies on a stream of its choice (fill_inputs_on)."""
import collections

import numpy as np

import autocorr_cases as ac
import bias_cases as bc
import density_cases as dc
import ergodic_cases as ec
import fan_cases as fc
import mixmoments_cases as mc
import predictive_cases as pc
import quantile_cases as qc
import score_cases as sc
from hmc_jl_amd import _lib

SENTINEL = -7.25
ISENTINEL = -7
F64, I64, I32 = np.float64, np.int64, np.int32

# An output block: its name, its shape with the windows first, its dtype and whether the call is given it (else a NULL pointer).
Out = collections.namedtuple("Out", "name shape dtype passed")
# A row of FEATURES.  call: the function of _lib; cases: the module of the reference and the bound; struct(case): the call's
# struct; inputs(case): [(name, array or None)] in pointer order; outputs(case): [Out] in pointer order; launches(case): what a
# timed call reports; unpack(case, blocks): what the feature's tests take as the result; reference(case) / check(case, result,
# ref, label): the feature's reference comparison; judged(case, ref): (reference arrays, bounds) for the CPU contract;
# stream_case(arrays, nd): the case of the stream tests on a dict of draw arrays; draws(seed, W, nd): that dict from `cases`.
Feature = collections.namedtuple("Feature", "name call cases struct inputs outputs launches unpack reference check judged stream_case draws")


def _dims(c, key="mu"):
    W, Cn, ld = c[key].shape
    return W, Cn, ld


def _need_A(horizons):
    return any(int(h) > 0 for h in horizons)


def flags_agree(got, exp_flag, exp_out, probs, tol):
    """Fan flags equal to the reference's wherever its decision has a margin: an item whose reference values put p within tol of
    Fhi, or Fhi - Flo within 2 tol of 0, may be flagged either way.  Returns (agree, items without margin)."""
    p = np.asarray(probs, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        Flo, Fhi = exp_out[..., 3], exp_out[..., 4]
        shaky = (np.abs(Fhi - Flo) <= 2.0 * tol) | (np.abs(p - Fhi) <= tol)
    nan_same = np.array_equal((got & fc.NAN_) != 0, (exp_flag & fc.NAN_) != 0)
    return nan_same and np.array_equal(got[~shaky], exp_flag[~shaky]), int(shaky.sum())


# ---- the settings of the stream tests (tests/test_gpu_stat_streams.py) ----------------------------------------------------------
K = 3
HORIZONS = (0, 12)                 # a horizon above 0: A is read
GRID = 65
BINS = 64
ROUNDS = 1
SCORE_STRIDE = 3                   # 689 used draws of 2065: 3 windows x (689 * 3)^2 pair terms, inside sc.PAIR_BUDGET
# name -> (W, nd, seed).  `large` is three slabs of PRED_SLAB draws, more windows and a larger arena for every feature that has
# one; small2 is small with another seed.
SHAPES = {"small": (1, 65, 11), "large": (3, 2065, 12), "small2": (1, 65, 13)}


def _mixture_draws(seed, W, nd):
    mu, sig2, pi, A = fc.make_draws(seed, W, K, nd, 0, True)
    return {"mu": mu, "sig2": sig2, "pi": pi, "A": A}


def panel_draws(seed, W, nd):
    """One set of draws every feature can run on: mu, sig2, pi, A, fcast (one horizon) and yreal (n_h, W)."""
    d = _mixture_draws(seed, W, nd)
    rng = np.random.default_rng(seed + 7)
    d["fcast"] = rng.normal(0.3, 1.5, size=(W, 2, nd))
    d["yreal"] = rng.normal(2.0, 3.0, size=(len(HORIZONS), W))
    return d


def _column(d):
    return d["x"] if "x" in d else d["mu"]


# ---- the nine rows ----------------------------------------------------------------------------------------------------------------

def _pred_struct(c):
    W, Kc, ld = _dims(c)
    return _lib.make_predictive(W, Kc, c["nd"], ld, len(c["grid"]), c["horizons"], 0, c["round5"])


def _pred_check(c, got, ref, label):
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref)), label
    err, tol = float(np.abs(got - ref).max()), pc.tolerance(c["nd"], c["mu"].shape[1], max(c["horizons"]))
    print("%s: max |diff| = %.3e, tol %.3e" % (label, err, tol))
    assert err <= tol, (label, err, tol)


PREDICTIVE = Feature(
    "predictive_cdf", "predictive_cdf_device", pc, _pred_struct,
    lambda c: [("mu", c["mu"]), ("sig2", c["sig2"]), ("pi", c["pi"]), ("A", c["A"]), ("grid", np.asarray(c["grid"], dtype=F64))],
    lambda c: [Out("cdf", (c["mu"].shape[0], len(c["horizons"]), len(c["grid"])), F64, True)],
    lambda c: 2,
    lambda c, b: b[0],
    lambda c: pc.reference(c["mu"], c["sig2"], c["pi"], c["A"], np.asarray(c["grid"], dtype=F64), c["horizons"], c["round5"], c["nd"]),
    _pred_check,
    lambda c, ref: ([ref], [pc.tolerance(c["nd"], c["mu"].shape[1], max(c["horizons"]))]),
    lambda d, nd: dict(mu=d["mu"], sig2=d["sig2"], pi=d["pi"], A=d["A"], grid=pc.make_grid(GRID), horizons=HORIZONS, nd=nd, round5=True),
    _mixture_draws)


def _bias_struct(c):
    W, Kc, ld = _dims(c)
    return _lib.make_bias(W, Kc, c["nd"], ld, c["horizon"], 0 if c["fc"] is None else c["fc"].shape[1] // 2, 0, c["round5"])


def _bias_draws(seed, W, nd):
    mu, pi, A, fcast = bc.make_draws(seed, W, K, nd, 0, True, 1)
    return {"mu": mu, "pi": pi, "A": A, "fcast": fcast}


BIAS = Feature(
    "bias_moments", "bias_moments_device", bc, _bias_struct,
    lambda c: [("mu", c["mu"]), ("pi", c["pi"]), ("A", c["A"] if c["horizon"] > 0 else None), ("fc", c["fc"])],
    lambda c: [Out("out", (c["mu"].shape[0], _lib.bias_stride(c["mu"].shape[1])), F64, True)],
    lambda c: 2,
    lambda c, b: (_lib.unpack_bias(b[0], c["mu"].shape[1]), b[0]),
    lambda c: bc.reference(c["mu"], c["pi"], c["A"], c["fc"], c["horizon"], c["round5"], c["nd"]),
    lambda c, got, ref, label: bc.check(got[0], ref, bc.tolerance(ref, c["nd"], c["mu"].shape[1], c["horizon"]), label),
    lambda c, ref: (lambda tol: ([ref[k] for k in tol], list(tol.values())))(bc.tolerance(ref, c["nd"], c["mu"].shape[1], c["horizon"])),
    lambda d, nd: dict(mu=d["mu"], pi=d["pi"], A=d["A"], fc=d["fcast"], horizon=max(HORIZONS), nd=nd, round5=True),
    _bias_draws)


def _mix_struct(c):
    W, Kc, ld = _dims(c)
    return _lib.make_mixmom(W, Kc, c["nd"], ld, c["hz"], 0, c["round5"])


MIX = Feature(
    "mixture_moments", "mixture_moments_device", mc, _mix_struct,
    lambda c: [("mu", c["mu"]), ("sig2", c["sig2"]), ("pi", c["pi"]), ("A", c["A"] if _need_A(c["hz"]) else None)],
    lambda c: [Out("out", (c["mu"].shape[0], len(c["hz"]), _lib.MIX_STRIDE), F64, True)],
    lambda c: 2,
    lambda c, b: (_lib.unpack_mixture_moments(b[0]), b[0]),
    lambda c: mc.reference(c["mu"], c["sig2"], c["pi"], c["A"], c["hz"], c["round5"], c["nd"]),
    lambda c, got, ref, label: mc.check(got[0], ref, mc.tolerance(ref, c["nd"], c["mu"].shape[1], c["hz"]), label),
    lambda c, ref: (lambda tol: ([ref[k] for k in tol], list(tol.values())))(mc.tolerance(ref, c["nd"], c["mu"].shape[1], c["hz"])),
    lambda d, nd: dict(mu=d["mu"], sig2=d["sig2"], pi=d["pi"], A=d["A"], hz=HORIZONS, nd=nd, round5=True),
    lambda seed, W, nd: dict(zip(("mu", "sig2", "pi", "A"), mc.make_draws(seed, W, K, nd, 0, True))))


def _dens_struct(c):
    W, Cn, ld = _dims(c, "x")
    return _lib.make_density(W, Cn, c["nd"], ld, c["cuts"], c["bins"], c["trace"], 0, c["round5"])


def _dens_outputs(c):
    W, Cn, _ = _dims(c, "x")
    nc, tl = len(c["cuts"]), int(c["trace"][0])
    return [Out("range", (W, Cn, 2), F64, True), Out("counts", (W, Cn, nc, c["bins"] + 3), I64, True),
            Out("stats", (W, Cn, nc, 2), F64, True), Out("trace", (W, Cn, max(tl, 1)), F64, tl > 0)]


def _dens_unpack(c, b):
    blocks = [b[0], b[1], b[2], b[3][:, :, :int(c["trace"][0])].copy()]
    return _lib.unpack_chain_density(*blocks), blocks


def _dens_judged(c, ref):
    tol = dc.tolerance(ref)
    return [ref[k] for k in tol], list(tol.values())


DENSITY = Feature(
    "chain_density", "chain_density_device", dc, _dens_struct,
    lambda c: [("x", c["x"]), ("lo_hi", None if c["lo_hi"] is None else np.asarray(c["lo_hi"], dtype=F64))],
    _dens_outputs,
    lambda c: 4 if c["lo_hi"] is None else 3,
    _dens_unpack,
    lambda c: dc.reference(c["x"], c["cuts"], c["bins"], c["lo_hi"], c["trace"], c["round5"], c["nd"]),
    lambda c, got, ref, label: dc.check(got[0], ref, label),
    _dens_judged,
    lambda d, nd: dict(x=_column(d), nd=nd, cuts=(nd,), bins=BINS, lo_hi=None, trace=(nd // 7, 7), round5=True),
    lambda seed, W, nd: {"x": dc.make_case(seed, W, K, nd, 0, BINS)})


def _acf_struct(c):
    W, Cn, ld = _dims(c, "x")
    return _lib.make_autocorr(W, Cn, c["nd"], ld, c["L"], 0, c["round5"])


def _acf_judged(c, ref):
    tol = ac.tolerance(ref)
    return [ref[k] for k in tol], list(tol.values())


AUTOCORR = Feature(
    "chain_autocorr", "chain_autocorr_device", ac, _acf_struct,
    lambda c: [("x", c["x"])],
    lambda c: [Out("acov", _dims(c, "x")[:2] + (c["L"] + 1,), F64, True), Out("diag", _dims(c, "x")[:2] + (_lib.ACF_STRIDE,), F64, True)],
    lambda c: 2,
    lambda c, b: _lib.unpack_chain_autocorr(b[0], b[1]),
    lambda c: ac.reference(c["x"], c["L"], c["round5"], c["nd"]),
    lambda c, got, ref, label: ac.check(got, ref, c["x"], c["round5"], c["nd"], label),
    _acf_judged,
    lambda d, nd: dict(x=_column(d), nd=nd, L=min(ac.LAG_EDGES), round5=True),
    lambda seed, W, nd: {"x": ac.make_case(seed, W, K, nd, 0)})


def _ord_struct(c):
    W, Cn, ld = _dims(c, "x")
    return _lib.make_quantiles(W, Cn, c["nd"], ld, c["probs"], 0, c["round5"])


QUANTILES = Feature(
    "chain_quantiles", "chain_quantiles_device", qc, _ord_struct,
    lambda c: [("x", c["x"])],
    lambda c: [Out("q", _dims(c, "x")[:2] + (len(c["probs"]), _lib.ORD_STRIDE), F64, True), Out("n", _dims(c, "x")[:2] + (2,), I64, True)],
    lambda c: 1,
    lambda c, b: _lib.unpack_chain_quantiles(b[0], b[1]),
    lambda c: qc.reference(c["x"], c["probs"], c["round5"], c["nd"]),
    lambda c, got, ref, label: qc.check(got, ref, label),
    lambda c, ref: ([ref[k] for k in qc.FIELDS], []),            # a selection: compared bit for bit, no bound
    lambda d, nd: dict(x=_column(d), nd=nd, probs=qc.PROBS3, round5=True),
    lambda seed, W, nd: {"x": qc.panel(seed, W, K, nd, 0)})


def _erg_struct(c):
    W, Kc, ld = _dims(c)
    return _lib.make_ergodic(W, Kc, c["nd"], ld, 0, c["round5"])


def _erg_outputs(c):
    W, Kc, ld = _dims(c)
    Cn = _lib.erg_cols(Kc)
    return [Out("cols", (W, Cn, ld), F64, bool(c["cols"])), Out("out", (W, Cn, 2), F64, True), Out("n", (W, 2), I64, True)]


def _erg_unpack(c, b):
    assert (b[0][:, :, c["nd"]:] == SENTINEL).all(), "wrote into the padding of cols"
    return (b[0] if c["cols"] else None), b[1], b[2]


def _erg_check(c, got, ref, label):
    cols, out, n = got
    cols = cols[:, :, :c["nd"]]
    assert ec.same_cells(cols, ref), (label, np.argwhere(ec.bits(cols) != ec.bits(ref))[:4])
    ec.check_pooled(out, n, cols, label)
    assert (n.sum(axis=1) == c["nd"]).all(), label


def _erg_judged(c, ref):
    pooled = ec.pooled_reference(ref)
    tol = ec.pooled_tolerance(pooled)
    return [pooled[k] for k in tol], list(tol.values())


ERGODIC = Feature(
    "ergodic_moments", "ergodic_moments_device", ec, _erg_struct,
    lambda c: [("mu", c["mu"]), ("sig2", c["sig2"]), ("A", c["A"])],
    _erg_outputs,
    lambda c: 2,
    _erg_unpack,
    lambda c: ec.panel_columns(c["mu"], c["sig2"], c["A"], c["nd"], c["round5"]),
    _erg_check,
    _erg_judged,
    lambda d, nd: dict(mu=d["mu"], sig2=d["sig2"], A=d["A"], nd=nd, round5=True, cols=True),
    lambda seed, W, nd: dict(zip(("mu", "sig2", "A"), ec.make_panel(seed, W, K, nd, 0))))


def _fan_struct(c):
    W, Kc, ld = _dims(c)
    return _lib.make_fan(W, Kc, c["nd"], ld, c["probs"], c["horizons"], c["rounds"], 0, c["round5"])


def _fan_outputs(c):
    W, n_h, n_p = c["mu"].shape[0], len(c["horizons"]), len(c["probs"])
    return [Out("out", (W, n_h, n_p, _lib.FAN_STRIDE), F64, True), Out("range", (W, 2), F64, True), Out("flag", (W, n_h, n_p), I32, True)]


def _fan_check(c, got, ref, label):
    out, rng, flag = got
    e_out, e_rng, e_flag = ref
    Kc = c["mu"].shape[1]
    assert np.array_equal(rng.view(np.uint64), e_rng.view(np.uint64)), (label, rng, e_rng)
    assert not (out == SENTINEL).any() and not (flag == ISENTINEL).any(), label
    ok, _ = flags_agree(flag, e_flag, e_out, c["probs"], fc.tolF(c["nd"], Kc, c["horizons"]))
    assert ok, (label, flag, e_flag)
    at = fc.judge(c["mu"], c["sig2"], c["pi"], c["A"], c["horizons"], c["round5"], c["nd"])
    return fc.check_block(out, rng, flag, c["probs"], c["horizons"], c["rounds"], c["nd"], Kc, at, label)


FAN = Feature(
    "predictive_quantiles", "predictive_quantiles_device", fc, _fan_struct,
    lambda c: [("mu", c["mu"]), ("sig2", c["sig2"]), ("pi", c["pi"]), ("A", c["A"])],
    _fan_outputs,
    lambda c: 2 + 2 * fc.rounds_of(c["rounds"]),
    lambda c, b: (b[0], b[1], b[2]),
    lambda c: fc.reference(c["mu"], c["sig2"], c["pi"], c["A"], c["probs"], c["horizons"], c["rounds"], c["round5"], c["nd"]),
    _fan_check,
    lambda c, ref: ([ref[0], ref[1]], [fc.tolF(c["nd"], c["mu"].shape[1], c["horizons"])]),
    lambda d, nd: dict(mu=d["mu"], sig2=d["sig2"], pi=d["pi"], A=d["A"], probs=fc.PROBS5, horizons=HORIZONS, rounds=ROUNDS, nd=nd, round5=True),
    _mixture_draws)


def _score_struct(c):
    W, Kc, ld = _dims(c)
    return _lib.make_score(W, Kc, c["nd"], ld, c["horizons"], c["stride"], 0, c["round5"])


def _score_check(c, got, ref, label):
    ref, bound = ref
    assert not (got == SENTINEL).any(), label
    worst = sc.worst_ratio(got, ref, bound)
    per = [sc.worst_ratio(got[..., i], ref[..., i], bound[..., i]) for i in range(5)]
    print("%s: max |device - ref| / bound = %.3g (%s)" % (label, worst, ", ".join("%s %.2g" % (n, v) for n, v in zip(sc.FIELDS, per))))
    assert worst <= 1.0, (label, got, ref, bound)
    return worst


def _score_draws(seed, W, nd):
    d = _mixture_draws(seed, W, nd)
    d["yreal"] = np.random.default_rng(seed + 7).normal(2.0, 3.0, size=(len(HORIZONS), W))
    return d


SCORES = Feature(
    "predictive_scores", "predictive_scores_device", sc, _score_struct,
    lambda c: [("mu", c["mu"]), ("sig2", c["sig2"]), ("pi", c["pi"]), ("A", c["A"]), ("yreal", np.asarray(c["yreal"], dtype=F64))],
    lambda c: [Out("out", (c["mu"].shape[0], len(c["horizons"]), _lib.SCORE_STRIDE), F64, True)],
    lambda c: 3,
    lambda c, b: b[0],
    lambda c: sc.reference(c["mu"], c["sig2"], c["pi"], c["A"], np.asarray(c["yreal"], dtype=F64), c["horizons"], c["stride"], c["round5"], c["nd"]),
    _score_check,
    lambda c, ref: ([ref[0]], [ref[1]]),
    lambda d, nd: dict(mu=d["mu"], sig2=d["sig2"], pi=d["pi"], A=d["A"], yreal=d["yreal"], horizons=HORIZONS, stride=SCORE_STRIDE, nd=nd,
                       round5=True),
    _score_draws)

FEATURES = collections.OrderedDict((f.name, f) for f in (PREDICTIVE, BIAS, MIX, DENSITY, AUTOCORR, QUANTILES, ERGODIC, FAN, SCORES))


def entry_symbol(feature):
    """The exported symbol behind a row."""
    return "hmcg_" + FEATURES[feature].call


def stream_case(feature, shape=None, draws=None, nd=None):
    """The case of the stream tests for `feature`: on SHAPES[shape], drawn by the feature's own *_cases module, or on `draws`
    (panel_draws, or a panel's fetched draws), nd draws each."""
    f = FEATURES[feature]
    if draws is None:
        W, nd, seed = SHAPES[shape]
        draws = f.draws(seed, W, nd)
    return f.stream_case(draws, nd)


# ---- one prepared call --------------------------------------------------------------------------------------------------------------

def _torch_dtype(torch, dt):
    return {F64: torch.float64, I64: torch.int64, I32: torch.int32}[dt]


class StatCall:
    """One statistic call's device buffers.  host: the inputs as contiguous arrays (None: a NULL pointer); dev: their device
    tensors; out: the framed output tensors, (W + 2, ...) each."""

    def __init__(self, feature, case, device=0):
        import torch
        _lib.load()
        self.torch, self.f, self.case = torch, FEATURES[feature], case
        self.device = torch.device("cuda", device)
        self.struct = self.f.struct(case)
        self.names = [n for n, _ in self.f.inputs(case)]
        self.host = [None if a is None else np.array(a, dtype=F64, order="C") for _, a in self.f.inputs(case)]        # copies: shared suites are read-only
        self.pinned = [None if a is None else torch.from_numpy(a).pin_memory() for a in self.host]
        self.dev = [None if a is None else torch.from_numpy(a).to(self.device) for a in self.host]
        self.outs = self.f.outputs(case)
        self.out = [torch.full((o.shape[0] + 2,) + tuple(o.shape[1:]), SENTINEL if o.dtype is F64 else ISENTINEL,
                               dtype=_torch_dtype(torch, o.dtype), device=self.device) for o in self.outs]
        self.timing = None

    def enqueue(self, stream=None, timed=False):
        """The library call on the prepared buffers and nothing else: no synchronisation before or after (a timed call waits
        inside the library).  stream: a torch.cuda.Stream (None: the library's own).  Returns the Timing struct or None."""
        ptrs = [0 if t is None else t.data_ptr() for t in self.dev]
        ptrs += [t[1:].data_ptr() if o.passed else 0 for o, t in zip(self.outs, self.out)]
        self.timing = getattr(_lib, self.f.call)(self.struct, *ptrs, None if stream is None else stream.cuda_stream, timed)
        return self.timing

    def fill_inputs_on(self, stream):
        """The host inputs into the device tensors by asynchronous copies (pinned memory) on `stream`: the host does not wait."""
        with self.torch.cuda.stream(stream):
            for t, p in zip(self.dev, self.pinned):
                if t is not None:
                    t.copy_(p, non_blocking=True)

    def poison_inputs(self):
        """NaN in every device input (on torch's current stream: synchronise before enqueueing)."""
        for t in self.dev:
            if t is not None:
                t.fill_(float("nan"))

    def collect(self):
        """Copies the outputs back, checks the sentinel frames and returns the unpacked result."""
        raw = [t.cpu().numpy() for t in self.out]
        for o, a in zip(self.outs, raw):
            s = SENTINEL if o.dtype is F64 else ISENTINEL
            assert (a[0] == s).all() and (a[-1] == s).all(), "%s: %s wrote outside its block" % (self.f.name, o.name)
            if not o.passed:
                assert (a == s).all(), "%s: wrote %s, which the call was not given" % (self.f.name, o.name)
        return self.f.unpack(self.case, [a[1:-1].copy() for a in raw])

    def reference(self):
        """The feature's reference for this case, computed once and kept in the case."""
        if "_ref" not in self.case:
            self.case["_ref"] = self.f.reference(self.case)
        return self.case["_ref"]

    def check(self, result, label=""):
        """The feature's own reference comparison, with its own bounds."""
        return self.f.check(self.case, result, self.reference(), label or self.f.name)


def prepare(feature, case, device=0):
    """Upload, allocate and prefill for one call; the StatCall comes back ready for .enqueue().  The uploads and fills run on
    torch's current stream: synchronise before enqueueing."""
    return StatCall(feature, case, device)


def run(feature, case, timed=True):
    """One stand-alone call on the library stream, as the nine feature modules make it: a timed call must report a positive
    kernel time and the row's launches; an untimed one is waited for here.  Returns the unpacked result."""
    c = prepare(feature, case)
    c.torch.cuda.synchronize(c.device)
    tm = c.enqueue(None, timed)
    if timed:
        assert tm.kernel_ms > 0.0 and tm.launches == c.f.launches(case), (feature, tm.kernel_ms, tm.launches)
    else:
        c.torch.cuda.synchronize(c.device)
    return c.collect()


# ---- bit comparisons between two results ----------------------------------------------------------------------------------------

def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def differing_fields(a, b, path=""):
    """The fields of two unpacked results (arrays, or tuples, lists and dicts of them, None allowed) that are not bit-equal."""
    if a is None or b is None:
        return [] if a is None and b is None else [path or "result"]
    if isinstance(a, dict):
        return ([path + "keys"] if set(a) != set(b) else []) + [p for k in a if k in b for p in differing_fields(a[k], b[k], "%s%s." % (path, k))]
    if isinstance(a, (tuple, list)):
        return ([path + "len"] if len(a) != len(b) else []) + [p for i, (x, y) in enumerate(zip(a, b)) for p in differing_fields(x, y, "%s%d." % (path, i))]
    a, b = np.asarray(a), np.asarray(b)
    same = a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))
    return [] if same else [path.rstrip(".") or "result"]


def assert_same_bits(a, b, label=""):
    bad = differing_fields(a, b)
    assert not bad, "%s: not bit-equal in %s" % (label, ", ".join(bad))
