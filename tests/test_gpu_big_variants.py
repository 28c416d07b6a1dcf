"""One oracle-parity case for EVERY instantiation of the LDS-resident kernel gibbs_sweeps_kernel_big<K, 256, SM, ST, SIG>.

csrc/variants.hpp (HMCG_BIG_FORM: the K list) and the variants_big*.hip units (g_big_xyz = HMCG_BIG_FORM(sig, smooth, stream))
define 8 forms x K = 2..8 = 56 separately compiled kernels; BIG (tests/kernel_tables.py) is parsed from those sources, so a new K or a new form
is picked up, and tests/test_variant_coverage.py (no GPU) holds the case lists to the tables.  Every case reaches its
kernel the way production does, without HMCG_FORCE_BIG / HMCG_FORCE_STREAM:
  * LDS-resident forms: the longest window lies beyond the register-resident ladder of its (K, path) -- 256 x the largest L of
    the parsed HMCG_V3 / HMCG_V rows, nothing at K >= 5 --, is no multiple of 256 and fits the LDS; the call also carries
    short windows (2 / 8, 64, 65, 257 steps), which make_plan then leaves on the same launch: the only production route by
    which the K <= 4 instantiations see short windows.  On the signal paths the shortest window has 8 steps (the shortest
    length the signal fuzz draws), every window holds its own signal range.
  * streaming forms: the longest window is beyond the LDS whatever the kernel's static share is (256 * 31 - 1 steps).
Bar, as everywhere (tests/oracle_parity.py): states bit-exact, floats within 1e-9 relative-to-(1+|x|), status 0, through the C ABI.  The call's own
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
import sys

import pytest

from hmc_jl_amd import _lib, synth
from kernel_tables import BIG, CSRC, KS, LDS_LIMIT, NT, ROOT, big_forms, coverage_lengths, dyn_bytes, form_id, ladder_ceiling
from oracle_parity import (SIGMA_SIGNAL, assert_ran_on_big, check_against_oracle, check_signals_against_oracle,
                           check_smoothing_against_oracle, signal_ranges)

pytestmark = pytest.mark.gpu


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


# ---- the coverage cases (kernel_tables.coverage_lengths, oracle_parity.signal_ranges) ----
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
