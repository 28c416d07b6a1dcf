"""The correlation kernels' test apparatus (tests/corr_cases.py), the parts that need no GPU: the ctypes mirror of MomentsArgs
against csrc/moments.hpp, the launchers' symbols in the built library, the table of draw_moments_kernel instantiations against
the K the GPU cases run, the kernel's pair decode, the long-double reference against the textbook formula, and the derived bound
on an fp64 stand-in of the kernels for every GPU case."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hmc_jl_amd

import corr_cases as cc
from kernel_tables import CSRC, ROOT
from density_cases import LD, round5

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_ctypes_struct_matches_the_header(tmp_path):
    fields = [f[0] for f in cc.MomentsArgs._fields_]
    src = tmp_path / "sz.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "%s"\nint main(){using A = hmcg_host::MomentsArgs;\n'
                   'std::printf("%%zu", sizeof(A));\n%s\nreturn 0;}\n'
                   % (os.path.join(CSRC, "moments.hpp"), "\n".join('std::printf(" %%zu", offsetof(A, %s));' % f for f in fields)))
    exe = tmp_path / "sz"
    subprocess.check_call(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(cc.MomentsArgs)] + [getattr(cc.MomentsArgs, f).offset for f in fields], (got, fields)
    assert got[0] == 80 and dict(zip(fields, got[1:])) == dict(mu=0, sig2=8, pi_end=16, A=24, fcast=32, mom=40, nd=48, nd_ld=56, W=64, K=68,
                                                               H=72, first=76)


def test_launcher_symbols_and_host_formulas():
    """The four symbols resolve in the built library; moments_stride and corr_columns (host functions) equal the Python formulas."""
    f = cc.bind(hmc_jl_amd.load())
    assert set(f) == {"launch_moments", "launch_corr_finalize", "moments_stride", "corr_columns"}
    for K in range(2, cc.MAXK + 1):
        assert f["corr_columns"](K) == cc.corr_columns(K) == 3 * K + K * K + 1
        NCp = cc.corr_columns(K) + 1
        assert f["moments_stride"](K) == cc.moments_stride(K) == cc.corr_columns(K) + NCp * (NCp + 1) // 2


def _gpu_case_ks():
    """The K of every case of the GPU suite that reaches draw_moments_kernel with a moment table the tests own."""
    import test_gpu_corr_kernels as t
    from test_variant_coverage import cases_of
    return {c[0] for c in cases_of(t.test_accumulation_and_finalisation)}


def test_moments_instantiation_table():
    """The HMCG_MOM(n) lines of launch_moments are {1, 2, 4, 8, 16}; PPT_OF_K follows from NP for every K; every compiled
    instantiation is the choice of some K the GPU cases run (no dead one) and every K has one (no missing one); K = HMCG_MAXK
    sits on the table's edge: 4095 of 4096 slots."""
    text = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "moments.hip")).read())
    body = text[text.index("hipError_t launch_moments"):]
    body = body[:body.index("#undef HMCG_MOM")]
    rows = [(int(a), int(b)) for a, b in re.findall(r"if\s*\(\s*ppt\s*<=\s*(\d+)\s*\)\s*HMCG_MOM\(\s*(\d+)\s*\)", body)]
    compiled = [int(n) for n in re.findall(r"\bHMCG_MOM\(\s*(\d+)\s*\)", body)]
    assert compiled == [1, 2, 4, 8, 16] == [b for _, b in rows] and all(a == b for a, b in rows), (compiled, rows)
    hdr = open(os.path.join(ROOT, "include", "hmcg.h")).read()
    maxk = int(re.search(r"#define\s+HMCG_MAXK\s+(\d+)", hdr).group(1))
    assert maxk == cc.MAXK and sorted(cc.PPT_OF_K) == list(range(2, maxk + 1))
    assert int(re.search(r"MOM_NT\s*=\s*(\d+)", text).group(1)) == cc.MOM_NT and int(re.search(r"MOM_TD\s*=\s*(\d+)", text).group(1)) == cc.MOM_TD
    for K in range(2, maxk + 1):
        need = (cc.n_pairs(K) + cc.MOM_NT - 1) // cc.MOM_NT
        pick = [b for a, b in rows if need <= a]
        assert pick, "K = %d has no instantiation" % K
        assert pick[0] == cc.PPT_OF_K[K] == cc.ppt_of(K), (K, need, pick)
        assert cc.n_pairs(K) <= pick[0] * cc.MOM_NT
    assert cc.n_pairs(maxk) == 4095 and max(compiled) * cc.MOM_NT == 4096
    ks = _gpu_case_ks()
    assert ks == set(range(2, maxk + 1))
    assert {cc.PPT_OF_K[K] for K in ks} == set(compiled), "an instantiation no GPU case runs, or one that is missing"
    import test_gpu_corr as abi
    from test_variant_coverage import cases_of
    assert {5, 6, 7} <= {c[0] for c in cases_of(abi.test_corr_matches_numpy)}          # <4>, <8>, <16> through the ABI as well


@pytest.mark.parametrize("K", range(2, cc.MAXK + 1))
def test_pair_decode_inverts_pair_index(K):
    """The kernel's decode loop over 0 .. NP - 1 hits every (i, j), i <= j, once, in pair_index's order."""
    NCp = cc.corr_columns(K) + 1
    NP = cc.n_pairs(K)
    seen = [cc.pair_decode(pr, NCp) for pr in range(NP)]
    assert sorted(seen) == [(i, j) for i in range(NCp) for j in range(i, NCp)] and len(set(seen)) == NP
    assert all(cc.pair_index(i, j, NCp) == pr for pr, (i, j) in enumerate(seen))
    assert cc.pair_index(NCp - 1, NCp - 1, NCp) == NP - 1
    mom = np.arange(cc.moments_stride(K), dtype=np.float64)
    piv, P = cc.unpack_mom(mom, NCp - 1)
    assert np.array_equal(piv, mom[:NCp - 1]) and all(P[i, j] == P[j, i] == NCp - 1 + pr for pr, (i, j) in enumerate(seen))


def test_reference_is_the_textbook_pearson_matrix():
    K, nd = 3, 200
    cols = cc.columns(*cc.make_case(7, 2, K, 3, nd, 5, "constant"))
    ref = cc.reference(cols, nd)
    x = round5(cols[:, :, :nd]).astype(LD)
    d = x - x.mean(axis=2, keepdims=True)
    cov = np.einsum("wid,wjd->wij", d, d)
    s = np.sqrt(np.einsum("wii->wi", cov))
    const = cc.constant_columns(cols, nd)
    assert const.sum() == 2 and const[:, K + 1].all()
    live = ~(const[:, :, None] | const[:, None, :])
    with np.errstate(invalid="ignore", divide="ignore"):
        text = cov / (s[:, :, None] * s[:, None, :])
        numpy64 = np.stack([np.corrcoef(round5(cols[w, :, :nd])) for w in range(2)])
    assert np.isnan(ref["r"][~live]).all() and np.isfinite(ref["r"][live].astype(np.float64)).all()          # NaN in its row and column only
    assert float(np.abs(ref["r"][live] - text[live]).max()) < 1e-16
    assert float(np.abs(ref["r"][live].astype(np.float64) - numpy64[live]).max()) < 1e-12
    assert (np.einsum("wii->wi", ref["r"])[~const] == 1).all()
    one = cc.reference(cols, 1)
    assert np.isnan(one["r"]).all() and cc.constant_columns(cols, 1).all()
    # the pair magnitudes of the bound
    _, _, a = cc.prepare(cols, nd)
    assert np.allclose(ref["A"][0, 0, 1], np.abs(a[0, 0] * a[0, 1]).sum()) and np.allclose(ref["B"][1, 2], np.abs(a[1, 2]).sum())


def test_finalize_restated_rules():
    """The diagonal rule, the clamp and the NaN of a constant column on a hand-made table."""
    NC = 2
    n = 4.0
    a = np.array([[0.0, 1.0, 2.0, 3.0], [0.0, 0.0, 0.0, 0.0]])
    v = np.vstack([a, np.ones(4)])
    P = v @ v.T
    mom = np.concatenate([[5.0, 6.0], P[np.triu_indices(3)]])
    r = cc.finalize_restated(mom, NC)
    assert P[2, 2] == n and r[0, 0] == 1.0 and np.isnan(r[0, 1]) and np.isnan(r[1, 0]) and np.isnan(r[1, 1])


def _stand_in_case(cols, nd, label, constant_allowed=True):
    ref = cc.reference(cols, nd)
    mom, corr = cc.stand_in(cols, nd)
    cc.check_table(mom, ref, label, fused=False)
    const = cc.constant_columns(cols, nd)
    if not constant_allowed:
        assert not const.any() or nd == 1, label
    return cc.check(corr, ref, label, constant=const), ref


@pytest.mark.parametrize("K,nd,W,H,pad", cc.accumulation_cases())
def test_bound_holds_on_the_stand_in_accumulation_cases(K, nd, W, H, pad):
    """Every GPU accumulation case: the fp64 stand-in (serial accumulation, finalize_restated) stays inside the bound, and the guard
    excludes nothing (at nd = 1 every column is constant)."""
    cols = cc.columns(*cc.make_case(cc.case_seed(K, nd), W, K, H, nd, pad, "plain"))
    assert cols.shape == (W, cc.corr_columns(K), nd + pad)
    _stand_in_case(cols, nd, "stand-in K=%d nd=%d" % (K, nd), constant_allowed=False)


@pytest.mark.parametrize("kind,K,W,H,nd,pad", cc.kind_cases())
def test_bound_holds_on_the_stand_in_kind_cases(kind, K, W, H, nd, pad):
    """Every GPU end-to-end case; the guard excludes the cells of the constant column of kind `constant` and nothing else."""
    arrays = cc.make_case(cc.case_seed(K, nd, kind), W, K, H, nd, pad, kind)
    assert np.isnan(arrays[4][:, 1:]).all() and all(np.isnan(a[..., nd:]).all() for a in arrays)
    cols = cc.columns(*arrays)
    const = cc.constant_columns(cols, nd)
    assert const.sum() == (W if kind == "constant" else 0)
    ratio, ref = _stand_in_case(cols, nd, "stand-in %s K=%d" % (kind, K))
    r = ref["r"].astype(np.float64)
    if kind == "duplicate":
        assert (np.abs(r[:, 0, 1] - 1.0) < 1e-15).all()
    if kind == "negated":
        assert (np.abs(r[:, 0, 1] + 1.0) < 1e-15).all()
    if kind == "collinear":
        assert (r[:, 0, 1] > 0.999999).all() and (r[:, 0, 1] < 1.0).all()
    if kind == "outlier":
        rho = cc.tolerance(ref)["rho"]                     # the cancellation case is really in the table
        assert (rho[:, 0] == rho.max(axis=1)).all() and (rho[:, 0] > 5.0 * np.median(rho, axis=1)).all()


@pytest.mark.parametrize("K,nd", cc.SPLIT_SHAPES + cc.SPLIT_ONES)
def test_bound_holds_on_the_stand_in_split_cases(K, nd):
    """The inputs of the block-split cases; every split sums to nd in two blocks or more."""
    cols = cc.columns(*cc.make_case(cc.case_seed(K, nd, "outlier"), 2, K, 3, nd, 0, "outlier"))
    _stand_in_case(cols, nd, "stand-in split K=%d nd=%d" % (K, nd), constant_allowed=False)
    for k, n, name in cc.split_cases():
        b = cc.split_blocks(n, name)
        assert sum(b) == n and len(b) >= 2 and min(b) >= 1, (k, n, name)
    assert {n for _, n, name in cc.split_cases() if name == "ones"} <= set(range(1, 66))


def test_checks_notice_a_subtly_wrong_result():
    """What the checks are for: a draw left out, a pair accumulated without its last draw, one cell off by 1e-11, a lost symmetry,
    a finite cell in a constant column's row, a diagonal one ulp from 1 each fail them."""
    K, nd = 5, 129
    cols = cc.columns(*cc.make_case(cc.case_seed(K, nd, "constant"), 1, K, 1, nd, 0, "constant"))
    ref = cc.reference(cols, nd)
    const = cc.constant_columns(cols, nd)
    mom, corr = cc.stand_in(cols, nd)
    cc.check(corr, ref, "intact", constant=const)
    short_mom, short = cc.stand_in(cols, nd - 1)
    with pytest.raises(AssertionError):
        cc.check(short, ref, "a draw short", constant=const)
    with pytest.raises(AssertionError):
        cc.check_table(short_mom, ref, "a draw short", fused=False)
    bad = mom.copy()
    NC = cc.corr_columns(K)
    _, _, a = cc.prepare(cols, nd)
    bad[0, NC + cc.pair_index(0, 3, NC + 1)] -= a[0, 0, -1] * a[0, 3, -1]
    with pytest.raises(AssertionError):
        cc.check_table(bad, ref, "one pair a draw short", fused=False)
    for i, j, delta in ((0, 3, 1e-11), (2, 7, -1e-11)):
        bad = corr.copy()
        bad[0, i, j] += delta
        bad[0, j, i] += delta
        assert abs(delta) < 1e-10
        with pytest.raises(AssertionError):
            cc.check(bad, ref, "one cell off", constant=const)
    bad = corr.copy()
    bad[0, 0, 3] = np.nextafter(bad[0, 0, 3], 2.0)
    with pytest.raises(AssertionError, match="symmetric"):
        cc.check(bad, ref, "asymmetric", constant=const)
    bad = corr.copy()
    bad[0, K + 1, 0] = bad[0, 0, K + 1] = 0.0
    with pytest.raises(AssertionError, match="NaN"):
        cc.check(bad, ref, "finite in a constant column", constant=const)
    bad = corr.copy()
    bad[0, 4, 4] = np.nextafter(1.0, 0.0)
    with pytest.raises(AssertionError, match="diagonal"):
        cc.check(bad, ref, "diagonal", constant=const)


def test_bound_at_the_largest_run_of_the_suite():
    """n = 1500 with the first draw 30 sd out: the derived bound passes the old 1e-10 there; the stand-in stays inside it."""
    K, nd = 2, 1500
    cols = cc.columns(*cc.make_case(3, 1, K, 1, nd, 0, "outlier"))
    ratio, ref = _stand_in_case(cols, nd, "stand-in outlier n=1500")
    tol = cc.tolerance(ref)
    assert 1e-10 < float(tol["corr"][tol["guard"]].max()) < 1e-9 and float(np.nanmax(tol["rho"])) < cc.GUARD
