"""One oracle-parity case for EVERY instantiation of the LDS-resident kernel gibbs_sweeps_kernel_big<K, 256, SM, ST, SIG>.

csrc/variants.hpp (HMCG_BIG_FORM: the K list) and the variants_big*.hip units (g_big_xyz = HMCG_BIG_FORM(sig, smooth, stream))
define 8 forms x K = 2..8 = 56 separately compiled kernels; BIG below is parsed from those sources, so a new K or a new form
is picked up, and tests/test_variant_coverage.py (no GPU) holds the case lists to the tables.  Every case reaches its
kernel the way production does, without HMCG_FORCE_BIG / HMCG_FORCE_STREAM:
  * LDS-resident forms: the longest window lies beyond the register-resident ladder of its (K, path) -- 256 x the largest L of
    the parsed HMCG_V3 / HMCG_V rows, nothing at K >= 5 --, is no multiple of 256 and fits the LDS; the call also carries
    short windows (2 / 8, 64, 65, 257 steps), which make_plan then leaves on the same launch: the only production route by
    which the K <= 4 instantiations see short windows.  On the signal paths the shortest window has 8 steps (the shortest
    length the signal fuzz draws), every window holds its own signal range.
  * streaming forms: the longest window is beyond the LDS whatever the kernel's static share is (256 * 31 - 1 steps).
Bar, as everywhere: states bit-exact, floats within 1e-9 relative-to-(1+|x|), status 0, through the C ABI.  The call's own
report proves which instantiation ran: occupancy 0 (the LDS-resident kernel), no helper waves, one bucket, 256 threads,
ceil(maxT / 256) steps per thread, the streaming flag, and lds_bytes on the right side of plan.hpp's `dyn` for that depth.

Then the base form at the depths where the kernel changes behaviour (the every-eight-steps rescale, the in-place four-row
products beyond eight steps): steps per thread 1, 2, 8, 9, 16, 17 at T = 256 L - 1, those of them the production dispatch gives
to this kernel; and the two lengths on either side of the LDS limit, computed as choose_big does (256 L 21 + 16 + static <=
160 KiB) with `static` read from the built code object's metadata (.group_segment_fixed_size in csrc/obj/*.s, as
tools/isa_lint.py reads it), or from a first call's lds_bytes - dyn where the build's assembly is not at hand.

For information (from the code-object metadata of this commit's build, not asserted as constants): static LDS of the base form and the
longest LDS-resident window,
    K        2      3      4      5      6      7      8
    static   19408  21776  24944  28880  33616  39120  45424  bytes
    L        26     26     25     25     24     23     22     steps per thread
    T        6656   6656   6400   6400   6144   5888   5632   steps (T + 1 streams)
No case is left out: the oracle serves all 56."""
import glob
import os
import re
import sys

import numpy as np
import pytest

from hmc_jl_amd import _lib, synth
from test_gpu_parity import TOL, check_against_oracle, check_signals_against_oracle, close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hmc.jl_amd", "csrc")
NT = 256
LDS_LIMIT = 160 * 1024                 # plan.hpp, choose_big: dynamic + static LDS of the instantiation must fit the CU's 160 KiB


def dyn_bytes(L):
    """plan.hpp's Plan::dyn of the LDS-resident forms at L steps per thread."""
    return NT * L * (8 + 8 + 4 + 1) + 16


def _code(path):
    """A source file without its // comments (a commented-out row is not an instantiation)."""
    return re.sub(r"//[^\n]*", "", open(path).read())


def _bool(s):
    return s == "true"


def register_rows():
    """Every register-resident instantiation (K, L, NT, sig, smooth, NH, OCC) of the variants_*.hip tables: the HMCG_V rows
    and the three flavours of each HMCG_V3 row, as variants.hpp expands them."""
    rows = []
    for fn in sorted(glob.glob(os.path.join(CSRC, "variants_*.hip"))):
        text = _code(fn)
        for m in re.finditer(r"HMCG_V3\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(true|false)\s*,\s*(true|false)\s*,", text):
            K, L, sig, sm = int(m.group(1)), int(m.group(2)), _bool(m.group(3)), _bool(m.group(4))
            rows += [(K, L, 256, sig, sm, 0, 1), (K, L, 256, sig, sm, 0, 2), (K, L, 256, sig, sm, 4, 2)]
        for m in re.finditer(r"HMCG_V\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(true|false)\s*,\s*(true|false)\s*,\s*(\d+)\s*,\s*(\d+)\s*,", text):
            rows.append((int(m.group(1)), int(m.group(2)), int(m.group(3)), _bool(m.group(4)), _bool(m.group(5)), int(m.group(6)), int(m.group(7))))
    return rows


def big_form_ks():
    """The K list of HMCG_BIG_FORM (variants.hpp): one HMCG_BIG(K, ...) per compiled K."""
    lines = open(os.path.join(CSRC, "variants.hpp")).read().split("\n")
    start = next(i for i, ln in enumerate(lines) if re.match(r"\s*#define\s+HMCG_BIG_FORM\b", ln))
    end = start
    while lines[end].rstrip().endswith("\\"):
        end += 1
    return [int(k) for k in re.findall(r"HMCG_BIG\(\s*(\d+)\s*,", "\n".join(lines[start:end + 1]))]


def big_forms():
    """{name digits 'xyz': (sig, smooth, stream)} of every g_big_xyz = HMCG_BIG_FORM(sig, smooth, stream) in variants_big*.hip."""
    forms = {}
    for fn in sorted(glob.glob(os.path.join(CSRC, "variants_big*.hip"))):
        for m in re.finditer(r"\bg_big_([01]{3})\s*=\s*HMCG_BIG_FORM\(\s*(true|false)\s*,\s*(true|false)\s*,\s*(true|false)\s*\)", _code(fn)):
            assert m.group(1) not in forms, "g_big_%s is defined twice" % m.group(1)
            forms[m.group(1)] = (_bool(m.group(2)), _bool(m.group(3)), _bool(m.group(4)))
    return forms


def big_instantiations():
    """(sig, smooth, stream, K) of every compiled gibbs_sweeps_kernel_big, in table order."""
    return [(sig, sm, st, K) for (sig, sm, st) in sorted(big_forms().values()) for K in big_form_ks()]


REG_ROWS = register_rows()
BIG = big_instantiations()
KS = big_form_ks()


def form_id(sig, smooth, stream):
    return "%d%d%d" % (sig, smooth, stream)


def ladder_ceiling(K, sig, smooth):
    """The longest window the register-resident kernels of (K, path) hold at 256 threads per window (0: there are none)."""
    return max([NT * L for (k, L, nt, s, m, _, _) in REG_ROWS if (k, nt, s, m) == (K, NT, sig, smooth)], default=0)


def test_big_table_shape():
    """8 forms x K = 2..8: the parser sees all 56, each g_big_xyz is the form its name says, and the ladder the cases are
    placed beyond is the parsed one."""
    forms = big_forms()
    assert sorted(forms) == ["%d%d%d" % (a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    for name, f in forms.items():
        assert name == form_id(*f), (name, f)
    assert KS == [2, 3, 4, 5, 6, 7, 8]
    assert len(BIG) == 56 and len(set(BIG)) == 56
    assert all(ladder_ceiling(K, False, False) == 0 for K in KS if K >= 5) and ladder_ceiling(3, False, False) >= 4096


# ---- what proves that the intended instantiation ran ----
def assert_ran_on_big(g, stream, maxT, sig=False, smooth=False):
    L = (maxT + NT - 1) // NT
    assert g["occupancy"] == 0, g["occupancy"]                       # the OCC template argument: 0 = the LDS-resident kernel
    assert g["helper_waves"] == 0 and g["buckets"] == 1
    assert g["threads_per_window"] == NT and g["steps_per_thread"] == L, (g["threads_per_window"], g["steps_per_thread"], L)
    assert g["streaming"] == stream
    if stream:
        assert 16 <= g["lds_bytes"] < dyn_bytes(L)                   # its per-step arrays are in HBM
    else:
        assert dyn_bytes(L) <= g["lds_bytes"] <= LDS_LIMIT
    assert ("sigvals" in g) == sig and ("pi_smooth_mean" in g) == smooth     # make_plan takes the path from the extras passed


# ---- the coverage cases ----
STREAM_T = NT * ((LDS_LIMIT - 16) // (NT * 21) + 1) - 1         # 7935: beyond the LDS even with no static share at all
SIG_LEN = (40, 1, None, 12, 40)                                   # per window: a tail, one step, everything a signal, tails
SAVE_LEN = (3, 1, 2, 3, 2)
SIGMA_SIGNAL = np.array([0.5, 1.0, 0.2, 0.8, 0.3])


def coverage_lengths(sig, smooth, stream, K):
    """Window lengths of the coverage case of one instantiation (longest first)."""
    top = STREAM_T if stream else max(ladder_ceiling(K, sig, smooth), 2 * NT) + NT + 45
    return [top, 8 if sig else 2, 64, 65, 257]


def signal_ranges(Tw):
    sig = np.array([[T - (T if n is None else n), T] for T, n in zip(Tw, SIG_LEN)], dtype=np.int32)
    save = np.array([[T - n, T] for T, n in zip(Tw, SAVE_LEN)], dtype=np.int32)
    return sig, save


def check_smoothing_against_oracle(oracle, Y, Tw, K, burnin, nrun, yreal, sig=None, ssig=None, n_samples=1,
                                   run=_lib.estimate_batch_host, **more):
    """extras.pi_smooth_mean / pi_filter_mean against the mean of the oracle's literal Pb recursion and its running filtered
    mean, with every other output; sig: on the signal path (as test_smoothed_means_on_the_signal_path_lds_resident_kernel)."""
    kw = dict(sig_range=sig, save_range=sig, sigma_signal=ssig, kappa=0.6, n_samples=n_samples, alpha=2.0, nu=2.0) if sig is not None else {}
    g = run(Y, Tw, K, burnin, nrun, (12,), yreal, want_state=True, want_smooth=True, want_filter_mean=True, **kw, **more)
    for w in range(Y.shape[0]):
        T = int(Tw[w])
        if sig is not None:
            o = oracle.estimate_signals(Y[w, :T], K, burnin, nrun, n_samples, sig=tuple(sig[w]), kappa=0.6, alpha=2.0, nu=2.0,
                                        sigma_signal=float(ssig[w]), save=tuple(sig[w]), yreal=yreal[w], window_id=w,
                                        want_smooth=True, want_filter_mean=True)
            assert close(g["sigvals"][w][:, :sig[w][1] - sig[w][0]], o["sigvals"]) < TOL
            fmean = o["pi_filter_mean"]
        else:
            o = oracle.estimate_window(Y[w, :T], K, burnin, nrun, (12,), yreal[w], window_id=w, want_smooth=True)
            fmean = oracle.estimate_signals(Y[w, :T], K, burnin, nrun, 1, horizons=(12,), yreal=yreal[w], window_id=w,
                                            want_filter_mean=True)["pi_filter_mean"]
        assert g["status"][w] == o["status"] == 0
        assert np.array_equal(g["x_final"][w, :T], o["x_final"]), "state path differs in window %d" % w
        assert close(g["mu"][w].T, o["mu"]) < TOL and close(g["sig2"][w].T, o["sig2"]) < TOL
        assert close(np.transpose(g["A"][w], (2, 1, 0)), o["A"]) < TOL and close(g["pi_end"][w].T, o["pi_end"]) < TOL
        assert close(g["fcast"][w].T, o["fcast"]) < TOL and close(g["summary"][w], o["summary"]) < TOL
        assert close(g["pif_final"][w, :T], o["pif_final"]) < TOL
        assert np.max(np.abs(g["pi_smooth_mean"][w, :T] - o["pi_smooth"].mean(axis=0))) < TOL, w
        assert np.max(np.abs(g["pi_filter_mean"][w, :T] - fmean)) < TOL, w
        assert np.max(np.abs(g["pi_smooth_mean"][w, :T].sum(axis=1) - 1)) < 1e-12
        if "pi_smooth_draws" in g:                               # asked for through `more`: samples.pib[Nrun, N, D] itself
            assert np.max(np.abs(np.transpose(g["pi_smooth_draws"][w, :, :T, :], (2, 1, 0)) - o["pi_smooth"])) < TOL, w
    return g


@pytest.mark.parametrize("sig,smooth,stream,K", BIG, ids=["%s-K%d" % (form_id(*c[:3]), c[3]) for c in BIG])
def test_every_big_instantiation_against_oracle(hmclib, oracle, sig, smooth, stream, K):
    lens = coverage_lengths(sig, smooth, stream, K)
    top = lens[0]
    assert top > ladder_ceiling(K, sig, smooth) and top % NT != 0
    Y, Tw, fut = synth.generate_panel(len(lens), top, K, ragged=lens)
    yreal = fut[:, 11:12]
    burnin, nrun = (1, 3) if stream and not sig else ((1, 2) if sig else (2, 4))     # signal paths: three chained noise samples
    if sig:
        rng, save = signal_ranges(Tw)
        if smooth:
            g = check_smoothing_against_oracle(oracle, Y, Tw, K, burnin, nrun, yreal, sig=rng, ssig=SIGMA_SIGNAL, n_samples=3)
        else:
            g = check_signals_against_oracle(oracle, Y, Tw, K, burnin, nrun, 3, rng, save, 0.6, 2.0, 2.0, SIGMA_SIGNAL, yreal)
    elif smooth:
        g = check_smoothing_against_oracle(oracle, Y, Tw, K, burnin, nrun, yreal)
    else:
        g = check_against_oracle(oracle, Y, Tw, K, burnin, nrun, (12,), yreal)
    assert (g["status"] == 0).all()
    assert_ran_on_big(g, stream, top, sig, smooth)


# ---- depth edges of the base form ----
DEPTHS = (1, 2, 8, 9, 16, 17)
DEPTH_CASES = [(K, L) for K in KS for L in DEPTHS if NT * L - 1 > ladder_ceiling(K, False, False)]


def test_depth_cases_are_those_the_dispatch_reaches():
    """Every depth at K >= 5; at K <= 4 only beyond the parsed ladder (today: 9 and up at K = 2 and 4, 17 and up at K = 3)."""
    for K in KS:
        mine = [L for (k, L) in DEPTH_CASES if k == K]
        assert mine == [L for L in DEPTHS if NT * L - 1 > ladder_ceiling(K, False, False)] and DEPTHS[-1] in mine, (K, mine)
        if ladder_ceiling(K, False, False) == 0:
            assert mine == list(DEPTHS)


@pytest.mark.parametrize("K,L", DEPTH_CASES, ids=["K%d-L%d" % c for c in DEPTH_CASES])
def test_base_form_depth_edges(hmclib, oracle, K, L):
    """T = 256 L - 1: every thread but the last holds L steps.  L = 8 / 9: the last depth without and the first with the
    in-place four-row products; 8 / 16 and 9 / 17: on and one past the every-eight-steps rescale."""
    T = NT * L - 1
    Y, Tw, fut = synth.generate_panel(1, T, K)
    g = check_against_oracle(oracle, Y, Tw, K, 1, 3, (1, 12), fut[:, [0, 11]])
    assert g["status"][0] == 0
    assert_ran_on_big(g, False, T)


# ---- capacity edge of the base form: the 160 KiB rule against the real kernels ----
def static_lds_from_build(K, sig=False, smooth=False, stream=False):
    """.group_segment_fixed_size of gibbs_sweeps_kernel_big<K, 256, smooth, stream, sig> in the build's own assembly
    (csrc/obj/*.s, kept by -save-temps), read by tools/isa_lint.py's metadata parser; None where the build left none."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_lint
    finally:
        sys.path.pop(0)
    want = "gibbs_big<%d,%d,%d,%d,%d>" % (K, NT, smooth, stream, sig)
    for path in sorted(glob.glob(os.path.join(CSRC, "obj", "variants_big*-hip-amdgcn-amd-amdhsa-gfx950.s"))):
        for k in isa_lint.lint_file(path)[1]:
            if isa_lint.demangle_short(k["name"]) == want:
                return int(k["lds"])
    return None


@pytest.mark.parametrize("K", KS, ids=["K%d" % K for K in KS])
def test_lds_capacity_edge(hmclib, oracle, K):
    """The longest window that still runs LDS-resident (it fills the dynamic LDS to the last byte the rule allows) and that
    length + 1 (the shortest streaming window): both ordinary shapes, both against the oracle at 1 + 2 sweeps."""
    static = static_lds_from_build(K)
    if static is None:                  # no assembly beside the library: what a first (LDS-resident) call reports
        Tp = max(ladder_ceiling(K, False, False), NT) + 1
        Yp, Twp, _ = synth.generate_panel(1, Tp, K)
        p = _lib.estimate_batch_host(Yp, Twp, K, 0, 1, (), None)
        assert not p["streaming"] and p["steps_per_thread"] == (Tp + NT - 1) // NT
        static = p["lds_bytes"] - dyn_bytes(p["steps_per_thread"])
    assert 0 < static < LDS_LIMIT
    Lmax = (LDS_LIMIT - 16 - static) // (NT * 21)
    assert dyn_bytes(Lmax) + static <= LDS_LIMIT < dyn_bytes(Lmax + 1) + static
    Tmax = NT * Lmax
    assert Tmax > ladder_ceiling(K, False, False)
    print("K=%d static LDS %d bytes, longest LDS-resident window %d steps (%d per thread)" % (K, static, Tmax, Lmax))
    for T, stream in ((Tmax, False), (Tmax + 1, True)):
        Y, Tw, fut = synth.generate_panel(1, T, K)
        g = check_against_oracle(oracle, Y, Tw, K, 1, 2, (12,), fut[:, 11:12])
        assert g["status"][0] == 0
        assert_ran_on_big(g, stream, T)
        assert g["streaming"] == stream, (T, g["lds_bytes"])
        if not stream:
            assert g["lds_bytes"] == static + dyn_bytes(Lmax), (g["lds_bytes"], static)      # the runtime's figure is the metadata's
