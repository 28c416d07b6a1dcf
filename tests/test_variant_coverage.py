"""The per-instantiation contract, checked without a GPU: every kernel instantiation the variant tables compile --
gibbs_sweeps_kernel<K, L, NT, SIG, SM, NH, OCC> (the three flavours of each HMCG_V3 row, the lone HMCG_V rows) and
gibbs_sweeps_kernel_big<K, 256, SM, ST, SIG> (8 forms x K = 2..8) -- is named by an oracle-parity case of the GPU suite, and no
case names a kernel that is not compiled.  The tables are parsed from csrc/variants.hpp and csrc/variants_*.hip and held
against the kernel symbols of the built libhmcgibbs.so, so that a regex which silently drops a row fails here; the cases are
the parametrize lists of the GPU tests themselves (importing those modules needs no GPU).

tests/sweep_identities.py's table (one sweep against the reference's formulas, on the oracle and on the GPU) is held to the same
parsed tables: every smoothing-capable form has a case there.

The device entry's contract is held the same way: every pointer member of hmcg_extras (parsed from include/hmcg.h) is passed by
some case of tests/test_gpu_device_entry.py, and its split-chain table covers every kernel form."""
import re

import device_entry
import kernel_tables as kt
import sweep_identities
import test_gpu_big_variants as big
import test_gpu_device_entry as dev
import test_gpu_parity as parity
import test_gpu_variants as reg
from hmc_jl_amd import _lib
from hmcg_header import extras_pointer_members

FLAVOUR, PATH = kt.FLAVOUR_WAVES, kt.PATH                               # (NH, OCC) of the three HMCG_V3 expansions; (sig, smooth) of a path


def fmt_reg(r):
    return "gibbs_sweeps_kernel<K=%d, L=%d, NT=%d, SIG=%d, SM=%d, NH=%d, OCC=%d>" % r


def fmt_big(b):
    sig, sm, st, K = b
    return "gibbs_sweeps_kernel_big<K=%d, 256, SM=%d, ST=%d, SIG=%d> (form %d%d%d)" % (K, sm, st, sig, sig, sm, st)


cases_of = kt.cases_of                                                  # a test's parametrize list: what the suite actually runs


def library_kernels():
    """The instantiations in the built library, from its kernel symbols (Itanium names: the template arguments are the
    Li<int>E / Lb<0|1>E fields, as tools/isa_lint.py reads them)."""
    names = kt.library_symbols(r"_ZN4hmcg\d+gibbs_sweeps_kernel(?:_big)?I\w+")
    regs, bigs = [], []
    for name in sorted(names):
        m = re.match(r"_ZN4hmcg\d+gibbs_sweeps_kernel(_big)?I((?:L[ib]\d+E)+)EEvNS_12KernelParamsE", name)
        assert m, "kernel symbol of an unknown shape: " + name
        a = kt.template_ints(m.group(2))
        if m.group(1):
            K, nt, sm, st, sig = a
            assert nt == 256, name
            bigs.append((bool(sig), bool(sm), bool(st), K))
        else:
            K, L, nt, sig, sm, nh, occ = a
            regs.append((K, L, nt, bool(sig), bool(sm), nh, occ))
    return regs, bigs


def test_parsed_tables_are_the_kernels_of_the_built_library():
    """129 register-resident and 56 LDS-resident instantiations today; whatever the numbers, the source parse and the
    library's symbols name the same kernels, none twice."""
    rows, bigs = kt.register_rows(), kt.big_instantiations()
    assert len(set(rows)) == len(rows) and len(set(bigs)) == len(bigs)
    lib_rows, lib_bigs = library_kernels()
    assert len(lib_rows) + len(lib_bigs) == len(rows) + len(bigs), (len(lib_rows), len(lib_bigs), len(rows), len(bigs))
    assert sorted(lib_rows) == sorted(rows), [fmt_reg(r) for r in set(lib_rows) ^ set(rows)]
    assert sorted(lib_bigs) == sorted(bigs), [fmt_big(b) for b in set(lib_bigs) ^ set(bigs)]
    assert len(bigs) == 56 and len(rows) >= 129


def covered_register_rows():
    """Instantiation -> the case that names it, over the register-resident case lists of the GPU suite."""
    named = {}
    for (K, L, path, fl) in cases_of(reg.test_every_variant_against_oracle):
        named[(K, L, 256) + PATH[path] + FLAVOUR[fl]] = "test_every_variant_against_oracle[K%d-L%d-%s-%s]" % (K, L, path, fl)
    for (K, L) in cases_of(reg.test_smoothed_and_filtered_means_on_the_signal_path):
        named[(K, L, 256, True, True, 0, 1)] = "test_smoothed_and_filtered_means_on_the_signal_path[K%d-L%d]" % (K, L)
    rows = kt.register_rows()
    for (K, L, nt) in parity.THREADS_PER_WINDOW_CASES:
        # a thread count of its own: the one base-path row of that (K, L, NT) is what threads_per_window=NT selects
        mine = [r for r in rows if r[:5] == (K, L, nt, False, False)]
        assert len(mine) <= 1, "several flavours at NT=%d: test_threads_per_window_variants_agree cannot tell them apart" % nt
        named[mine[0] if mine else (K, L, nt, False, False, -1, -1)] = "test_threads_per_window_variants_agree (K=%d L=%d NT=%d)" % (K, L, nt)
    return named


def test_every_register_resident_instantiation_has_an_oracle_case():
    rows, named = set(kt.register_rows()), covered_register_rows()
    missing = sorted(rows - set(named))
    assert not missing, "compiled, but no oracle-parity case names it: " + "; ".join(fmt_reg(r) for r in missing)
    extra = sorted(set(named) - rows)
    assert not extra, "a case names a kernel that is not compiled: " + "; ".join("%s -> %s" % (named[r], fmt_reg(r)) for r in extra)


def test_every_lds_resident_instantiation_has_an_oracle_case():
    bigs = set(kt.big_instantiations())
    cases = cases_of(big.test_every_big_instantiation_against_oracle)
    assert len(set(cases)) == len(cases)
    missing = sorted(bigs - set(cases))
    assert not missing, "compiled, but no oracle-parity case names it: " + "; ".join(fmt_big(b) for b in missing)
    extra = sorted(set(cases) - bigs)
    assert not extra, "a case names a kernel that is not compiled: " + "; ".join(fmt_big(b) for b in extra)
    # the coverage case must take the production route to its kernel: beyond the ladder (LDS forms) / beyond the LDS (streaming)
    for (sig, sm, st, K) in cases:
        top = kt.coverage_lengths(sig, sm, st, K)[0]
        assert top > kt.ladder_ceiling(K, sig, sm) and top % 256 != 0, fmt_big((sig, sm, st, K))
        assert (kt.dyn_bytes((top + 255) // 256) > kt.LDS_LIMIT) == st, fmt_big((sig, sm, st, K))


def test_depth_cases_stay_beyond_the_ladder():
    """The fixed depth cases of the base form only name depths the production dispatch hands to the LDS-resident kernel, and
    every K has its deepest ones."""
    cases = cases_of(big.test_base_form_depth_edges)
    for (K, L) in cases:
        assert 256 * L - 1 > kt.ladder_ceiling(K, False, False), (K, L)
    for K in kt.big_form_ks():
        assert {L for (k, L) in cases if k == K} >= {L for L in (8, 9, 16, 17) if 256 * L - 1 > kt.ladder_ceiling(K, False, False)}, K
        assert (K, 17) in cases


# ---- the device entry (tests/test_gpu_device_entry.py) ----
def test_extras_parse_matches_the_ctypes_binding():
    import ctypes
    ptrs = extras_pointer_members()
    assert ptrs == [n for n, t in _lib.Extras._fields_ if t is ctypes.c_void_p]
    assert len(ptrs) >= 16 and len(set(ptrs)) == len(ptrs)
    # what the runner reports as passed is read from the struct it builds: a bare call passes none, a full one every member
    import numpy as np
    Y, T = np.zeros((2, 8)), np.array([8, 8])
    assert device_entry.extras_passed(Y, T, 3, 1, 2) == set()
    sig = np.array([[4, 8], [4, 8]])
    full = dict(x_init=np.zeros((2, 8)), want_state=True, window_ids=[0, 1], sig_range=sig, save_range=sig, sigma_signal=[1.0, 1.0],
                end_pos=[7, 7], want_sample_summary=True, want_smooth=True, want_filter_mean=True, want_smooth_draws=True, want_corr=True)
    assert device_entry.extras_passed(Y, T, 3, 1, 2, **full) == set(ptrs)
    assert "pif_final" not in device_entry.extras_passed(Y, T, 3, 1, 2, want_smooth=True, pass_pif=False)


def test_every_extras_pointer_is_passed_on_the_device_entry():
    """The runner builds each case's hmcg_extras with the code it runs on the GPU (over placeholder addresses) and the members
    it sets are read from the struct.  A new member of hmcg_extras without a device-entry case fails here."""
    cases = cases_of(dev.test_device_entry_against_oracle)
    assert cases == dev.PARITY_CASES and cases_of(dev.test_fresh_call_ignores_buffer_contents) == dev.PARITY_CASES
    passed = {}
    for c in cases:
        args, kw = dev.call_of(c)
        got = device_entry.extras_passed(*args, **kw, **dev.device_kw(c))
        assert got == dev.case_extras(c), c["id"]
        for f in got:
            passed.setdefault(f, c["id"])
    missing = [f for f in extras_pointer_members() if f not in passed]
    assert not missing, "no device-entry case passes extras." + ", extras.".join(missing)


def test_device_entry_parity_cases_cover_every_family_and_path():
    have = {(c["kernel"], c["path"]) for c in dev.PARITY_CASES}
    want = {(k, "base") for k in ("register", "lds", "stream")} | {(k, p) for k in ("register", "lds") for p in ("sig", "tail", "smooth", "teacher")}
    want.add(("stream", "smooth"))
    assert want <= have, sorted(want - have)
    assert any(c["bucketed"] for c in dev.PARITY_CASES) and any(c["kernel"] == "register" and not c["bucketed"] and len(set(c["lens"])) > 1 for c in dev.PARITY_CASES)
    for c in dev.PARITY_CASES:
        sig, smooth = c["path"] in ("sig", "tail"), c["path"] == "smooth"
        top = max(c["lens"])
        if c["kernel"] == "register":
            assert top <= kt.ladder_ceiling(c["K"], sig, smooth), c["id"]
        else:                                                  # the production route to the LDS-resident kernel and its streaming form
            assert top > kt.ladder_ceiling(c["K"], sig, smooth), c["id"]
            assert (kt.dyn_bytes((top + 255) // 256) > kt.LDS_LIMIT) == (c["kernel"] == "stream"), c["id"]


def test_split_chain_table_covers_every_kernel_form():
    cases = cases_of(dev.test_split_chain_equals_one_launch)
    assert cases == dev.SPLIT_CASES
    forms = {c["form"] for c in cases}
    assert forms >= {"register", "lds", "streaming", "sig", "sm", "sig+sm"}, sorted(forms)
    carried = set()
    for c in cases:
        args, kw = dev.call_of(c)
        sig, smooth = "sig_range" in kw, "want_smooth" in kw
        assert (c["form"] in ("sig", "sig+sm")) == sig and (c["form"] in ("sm", "sig+sm")) == smooth, c["id"]
        if c["kernel"] == "register":
            assert max(c["lens"]) <= kt.ladder_ceiling(c["K"], sig, smooth), c["id"]
        else:
            assert max(c["lens"]) > kt.ladder_ceiling(c["K"], sig, smooth) or ("HMCG_FORCE_BIG", "1") in c["env"], c["id"]
        burnin, nrun = c["sweeps"]
        per = burnin + nrun
        # the cuts the issue of this table asks for: inside burn-in, exactly at burnin, after a kept draw, a three-piece run;
        # on the signal path inside a sample before / after its first kept draw, at a sample boundary, inside a later sample
        cuts = {s for sp in c["splits"] for s in sp}
        assert any(0 < s < burnin for s in cuts) and any(len(sp) == 2 for sp in c["splits"]) or sig, c["id"]
        if sig:
            assert any(s < burnin for s in cuts) and any(burnin < s < per for s in cuts) and any(s % per == 0 for s in cuts) and any(s > per and s % per > burnin for s in cuts), c["id"]
        else:
            assert burnin in cuts and any(s > burnin for s in cuts), c["id"]
        carried |= device_entry.extras_passed(*args, **kw) & set(device_entry.CARRIED)
    assert carried == set(device_entry.CARRIED) - {"status"}, sorted(carried)
    assert {v for c in cases for k, v in c["env"] if k == "HMCG_FLAVOUR"} == set(FLAVOUR)


# ---- one sweep against the reference's formulas (tests/sweep_identities.py) ----
def test_sweep_identity_cases_cover_every_smoothing_form():
    """A SM or SIG + SM row, or a smoothing form of the LDS-resident kernel, that is added to the variant tables without a case in
    sweep_identities.CASES fails here; so does a case that names a row which is not compiled, or whose windows the production
    dispatch would hand to another kernel."""
    rows, cases = kt.register_rows(), sweep_identities.CASES
    reg = [c for c in cases if c["kernel"] == "register"]
    # every SM register row's (K, L); the flavours a case forces are compiled
    sm_rows = {(K, L) for (K, L, nt, sig, sm, _, _) in rows if (nt, sig, sm) == (256, False, True)}
    named = {(c["K"], c["L"]) for c in reg if c["path"] == "smooth"}
    assert sm_rows and sm_rows <= named, "SM rows without a sweep-identity case: %s" % sorted(sm_rows - named)
    for c in reg:
        sig = c["path"] != "smooth"
        if c["flavour"]:
            assert (c["K"], c["L"], 256, sig, True) + FLAVOUR[c["flavour"]] in rows, c["id"]
        else:
            assert sig and [r[5:] for r in rows if r[:5] == (c["K"], c["L"], 256, True, True)] == [(0, 1)], c["id"]
        classes = sorted({L for (K, L, nt, s, m, _, _) in rows if (K, nt, s, m) == (c["K"], 256, sig, True)})
        for T in c["lens"]:                                   # every window selects the row the case names: one launch, no buckets
            assert min(L for L in classes if 256 * L >= T) == c["L"], (c["id"], T)
    assert {fl for c in reg if c["path"] == "smooth" and c["L"] in (1, 4) for fl in [c["flavour"]]} == set(FLAVOUR)
    assert any(c["flavour"] == "h" and any(769 <= T <= 1024 for T in c["lens"]) for c in reg)
    # every SIG + SM register row's K
    sigsm_ks = {K for (K, L, nt, sig, sm, _, _) in rows if (nt, sig, sm) == (256, True, True)}
    named_ks = {c["K"] for c in reg if c["path"] != "smooth"}
    assert sigsm_ks and sigsm_ks <= named_ks, "SIG + SM rows without a sweep-identity case: K = %s" % sorted(sigsm_ks - named_ks)
    # each smoothing form of the LDS-resident kernel, reached the way production reaches it
    forms = {}
    for c in cases:
        if c["kernel"] != "register":
            sig, stream, top = c["path"] != "smooth", c["kernel"] == "stream", max(c["lens"])
            assert (sig, True, stream, c["K"]) in kt.big_instantiations(), c["id"]
            assert top > kt.ladder_ceiling(c["K"], sig, True) and top % 256 != 0, c["id"]
            assert (kt.dyn_bytes((top + 255) // 256) > kt.LDS_LIMIT) == stream, c["id"]
            forms.setdefault((sig, True, stream), c["id"])
    smoothing_forms = {f for f in kt.big_forms().values() if f[1]}
    assert len(smoothing_forms) == 4 and smoothing_forms <= set(forms), sorted(smoothing_forms - set(forms))
    # the tail path (end_pos with smoothing outputs) on a register form, an LDS form and a streaming form
    assert {c["kernel"] for c in cases if c["path"] == "tail+smooth"} == {"register", "lds", "stream"}
    for id in sweep_identities.MULTI_SAMPLE + sweep_identities.DEVICE_ENTRY:
        assert sweep_identities.case_by_id(id)["path"] == "tail+smooth"
    assert [sweep_identities.case_by_id(id)["kernel"] for id in sweep_identities.MULTI_SAMPLE] == ["register", "lds", "stream"]
    assert [sweep_identities.case_by_id(id)["kernel"] for id in sweep_identities.DEVICE_ENTRY] == ["register", "lds"]
