"""The branch contract of tests/test_gpu_branches.py, checked without a GPU.

test_variant_coverage.py guarantees that every kernel instantiation is NAMED by an oracle-parity case; this module guarantees
that, per instantiation, one of those cases drives the sampler through a permuted label order, and that every rare draw
branch is reached where its code lives.  It runs the oracle alone on each case's inputs (tests/branch_cases.py builds them for
both modules) and reads the oracle's branch counters (out["branches"]):

  * a mixed-label case: status 0, a non-identity sortperm(mu) on at least a third of the kept sweeps, and for K >= 3 at least
    one kept sweep whose order is not its own inverse (a swap equals its inverse, so only a longer cycle can tell a gather
    through `order` from one through its inverse);
  * a directed case: each branch it is listed for is taken at least once, status 0;
  * the mixed-label list names exactly the instantiations of csrc/variants_*.hip, as test_variant_coverage.py derives them:
    a new table row without a mixed-label case fails here.

What this does not guarantee: that the GPU takes the same branch for the same reason -- that is the parity test's business, on
the GPU -- nor any branch the counters do not list.  Cost: the oracle runs 3 to 8 sweeps per case; 214 tests in 3.5 s where
the parent commit's whole `-m "not gpu"` suite takes 7 min 7 s."""
import pytest

import branch_cases as bc
import kernel_tables as kt
import test_gpu_big_variants as big
import test_gpu_branches as gpu
import test_variant_coverage as cov

MIXED = gpu.MIXED
DIRECTED = gpu.DIRECTED


def instantiation_of(c):
    """The kernel a mixed-label case selects, in the tuples of kt.register_rows() / kt.big_instantiations()."""
    if c.kind == "reg":
        K, L, path, fl = c.expect
        return (K, L, 256) + kt.PATH[path] + kt.FLAVOUR_WAVES[fl]
    if c.kind == "sigsmooth":
        K, L = c.expect
        return (K, L, 256, True, True, 0, 1)
    if c.kind == "tpw":
        K, L, nt = c.expect
        mine = [r for r in kt.register_rows() if r[:5] == (K, L, nt, False, False)]
        return mine[0] if len(mine) == 1 else (K, L, nt, False, False, -1, -1)
    return tuple(c.expect)


def test_the_gpu_module_runs_these_lists():
    """The parametrize lists of the GPU tests are the lists held to the contract here."""
    assert list(cov.cases_of(gpu.test_mixed_labels_in_every_instantiation)) == MIXED
    assert list(cov.cases_of(gpu.test_directed_draw_branches)) == DIRECTED
    assert len({c.id for c in MIXED + DIRECTED}) == len(MIXED) + len(DIRECTED)


def test_mixed_label_list_is_the_instantiation_set():
    rows, bigs = set(kt.register_rows()), set(kt.big_instantiations())
    named = [instantiation_of(c) for c in MIXED]
    assert len(set(named)) == len(named), "two mixed-label cases name one kernel"
    regs = {n for n in named if len(n) == 7}
    lds = {n for n in named if len(n) == 4}
    missing = sorted(rows - regs)
    assert not missing, "compiled, but no mixed-label case: " + "; ".join(cov.fmt_reg(r) for r in missing)
    assert not sorted(regs - rows), "a mixed-label case names a kernel that is not compiled: %r" % sorted(regs - rows)
    assert not sorted(bigs - lds), "compiled, but no mixed-label case: " + "; ".join(cov.fmt_big(b) for b in sorted(bigs - lds))
    assert not sorted(lds - bigs), "a mixed-label case names a kernel that is not compiled: %r" % sorted(lds - bigs)
    # ... the very set test_variant_coverage.py holds the per-instantiation cases to
    assert regs == set(cov.covered_register_rows()) and lds == set(cov.cases_of(big.test_every_big_instantiation_against_oracle))


def test_mixed_label_cases_select_their_kernel_by_length():
    """The window of a register-resident case lies in its steps-per-thread class alone; an LDS-resident case takes the production
    route (beyond the ladder, beyond the LDS for the streaming forms)."""
    for c in MIXED:
        if c.kind in ("reg", "sigsmooth"):
            K, L = c.expect[:2]
            path = (c.sig, c.smooth)
            below = [l for (k, l, nt, s, m, _, _) in kt.register_rows() if (k, nt, s, m) == (K, 256) + path and l < L]
            assert 256 * max(below, default=0) < c.T <= 256 * L and c.T >= 2, c.id
        elif c.kind == "big":
            sig, sm, st, K = c.expect
            assert c.T > kt.ladder_ceiling(K, sig, sm) and (kt.dyn_bytes((c.T + 255) // 256) > kt.LDS_LIMIT) == st, c.id


@pytest.mark.parametrize("case", MIXED, ids=[c.id for c in MIXED])
def test_mixed_label_case_permutes_labels_on_the_oracle(oracle, case):
    o = bc.run_oracle(oracle, case)
    miss = bc.mixed_conditions(case, o["branches"], o["status"])
    assert not miss, "%s: %s" % (case.id, "; ".join(miss))


@pytest.mark.parametrize("case", DIRECTED, ids=[c.id for c in DIRECTED])
def test_directed_case_reaches_its_branch_on_the_oracle(oracle, case):
    o = bc.run_oracle(oracle, case)
    assert o["status"] == 0 and case.branches
    miss = bc.directed_conditions(case, o["branches"], o["status"])
    assert not miss, "%s (seed %d, window %d): %s" % (case.id, case.seed, case.window_id, "; ".join(miss))


def test_directed_table_covers_every_branch_in_every_place():
    """Each listed branch in each place the draw code lives: three flavours of the register-resident kernel, the LDS-resident
    kernel's LDS and streaming forms; the empty state at 1000 steps or more; the uniform fallback in the two families that
    no other test takes it in (test_gpu_k8_edges.py takes it on the LDS-resident kernel)."""
    def place(c):
        return c.expect[3] if c.kind == "reg" else ("stream" if c.expect[2] else "lds")
    want = ("gamma_3plus_sig2", "gamma_3plus_A", "v_rejects", "shape_lt1", "empty_states", "sig_only_states", "real_only_states")
    for pl in ("p1", "p2", "h", "lds", "stream"):
        mine = [c for c in DIRECTED if place(c) == pl]
        reached = {b for c in mine for b in c.branches}
        assert reached >= set(want), (pl, sorted(set(want) - reached))
        assert any("empty_states" in c.branches and c.T >= 1000 for c in mine), pl
        assert any("shape_lt1" in c.branches and 0 < c.alpha < 1 for c in mine), pl
        assert all(c.sig for c in mine if "sig_only_states" in c.branches), pl
        if pl != "lds":
            assert "x_uniform_fallbacks" in reached, pl
    assert {c.K for c in DIRECTED if c.kind == "big"} >= {5, 8} and all(c.K <= 4 for c in DIRECTED if c.kind == "reg")
