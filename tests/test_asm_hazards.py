"""tools/asm_hazards.py: the gfx950 wait states around and inside inline assembly (the compiler pads nothing there).

One snippet per rule that must be flagged and its padded twin that must pass; the eps() guard of the K = 8 filter replay as it
was generated until it compared into eight masks; a VCC write at the end of a loop that reaches a read at its top through the
back-edge; and, on the built csrc/obj/*.s, zero findings in every asm region and zero in the compiler's own code (the
calibration: the compiler pads its code correctly, so a finding there would mean the rule table is wrong)."""
import glob
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "hmc.jl_amd", "csrc", "obj")
TOOL = os.path.join(ROOT, "tools", "asm_hazards.py")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import asm_hazards  # noqa: E402


def kernel(body):
    """a kernel whose body is one asm region, led and closed by compiler code"""
    return ("_Z4kernv:\n\ts_load_dwordx2 s[0:1], s[4:5], 0x0\n\ts_waitcnt lgkmcnt(0)\n\ts_nop 4\n\t;;#ASMSTART\n"
            + "".join(ln + "\n" for ln in body) + "\t;;#ASMEND\n\ts_nop 4\n\ts_endpgm\n.Lfunc_end0:\n")


# rule -> (producer, consumer, the wait states the rule needs); each case is flagged as is and passes with the pad in between
CASES = {
    "valu-sgpr>valu": ("v_cmp_lt_i32 vcc, v1, v2", "v_cndmask_b32 v3, v4, v5, vcc", 2),
    "valu-sgpr>valu carry": ("v_add_co_u32 v1, vcc, v2, v3", "v_addc_co_u32 v4, s[8:9], 0, v5, vcc", 2),
    "valu-sgpr>valu operand": ("v_readfirstlane_b32 s10, v1", "v_add_u32 v2, s10, v3", 2),
    "valu-sgpr>vmem": ("v_readfirstlane_b32 s11, v1", "global_load_dword v2, v3, s[10:11]", 5),
    "valu-sgpr>lanesel": ("v_readfirstlane_b32 s12, v1", "v_readlane_b32 s13, v2, s12", 4),
    "valu-sgpr>lanesel writelane": ("v_cmp_eq_u32 s[12:13], v1, v2", "v_writelane_b32 v3, 7, s12", 4),
    "valu-vcc>div_fmas": ("v_div_scale_f64 v[0:1], vcc, v[2:3], v[2:3], v[4:5]", "v_div_fmas_f64 v[6:7], v[8:9], v[10:11], v[12:13]", 4),
    "valu-vgpr>dpp": ("v_add_u32 v1, v2, v3", "v_add_u32_dpp v4, v1, v4 row_shr:1 row_mask:0xf bank_mask:0xf", 2),
    "valu-exec>dpp": ("v_cmpx_lt_i32 vcc, v1, v2", "v_mov_b32_dpp v4, v5 row_shr:1 row_mask:0xf bank_mask:0xf", 5),
    "valu-vgpr>readlane": ("v_add_u32 v1, v2, v3", "v_readfirstlane_b32 s14, v1", 1),
    "valu-vgpr>permlane": ("v_add_u32 v2, 1, v1", "v_permlane32_swap_b32 v1, v2", 2),
    "trans>valu": ("v_rcp_f64 v[0:1], v[2:3]", "v_add_f64 v[4:5], v[0:1], 1.0", 1),
}


def findings(tmp_path, text, *flags):
    p = tmp_path / "t.s"
    p.write_text(text)
    return asm_hazards.check_file(str(p), outside="--outside" in flags)


@pytest.mark.parametrize("case", sorted(CASES))
def test_each_rule_flags_the_bare_pair_and_passes_the_padded_one(tmp_path, case):
    prod, cons, w = CASES[case]
    rule = case.split()[0]
    bad = findings(tmp_path, kernel(["s_nop 4", prod, cons]))
    assert [f[2] for f in bad] == [rule], (case, bad)
    assert bad[0][3] == 0 and bad[0][4] == w
    # one wait state short: still flagged (s_nop N counts N + 1); exactly enough: clean
    if w > 1:
        short = findings(tmp_path, kernel(["s_nop 4", prod, "s_nop %d" % (w - 2), cons]))
        assert [f[2] for f in short] == [rule], (case, short)
    assert findings(tmp_path, kernel(["s_nop 4", prod, "s_nop %d" % (w - 1), cons])) == [], case
    # independent instructions count like s_nop
    fill = ["s_mov_b32 s40, 0"] * w
    assert findings(tmp_path, kernel(["s_nop 4", prod] + fill + [cons])) == [], case


def test_the_replay_eps_guard_as_it_was_generated_is_flagged(tmp_path):
    """csrc/replay_asm_k8.inc before the fix: each v_cndmask read the vcc that the v_cmp right above it had written (the
    stale mask of the previous label where pif[t, s-1] and pif[t, s] straddle eps())."""
    body = ["s_nop 4", "s_mov_b32 s18, 0", "s_mov_b32 s19, 0x3cb00000", "v_mov_b32 v217, 0"]
    for s in range(8):
        body += ["v_cmp_lt_f64 vcc, s[18:19], v[%d:%d]" % (2 * s, 2 * s + 1),
                 "v_cndmask_b32 v219, v%d, v220, vcc" % (226 + s), "v_or_b32 v217, v217, v219"]
    bad = findings(tmp_path, kernel(body))
    assert len(bad) == 8 and {f[2] for f in bad} == {"valu-sgpr>valu"}
    # the fixed form: eight compares into eight masks, then the selects
    masks = ["s[20:21]", "s[22:23]", "s[24:25]", "s[26:27]", "s[28:29]", "s[30:31]", "s[34:35]", "s[16:17]"]
    body = ["s_nop 4", "s_mov_b32 s18, 0", "s_mov_b32 s19, 0x3cb00000"]
    body += ["v_cmp_lt_f64 %s, s[18:19], v[%d:%d]" % (masks[s], 2 * s, 2 * s + 1) for s in range(8)]
    body += ["v_cndmask_b32 v217, v226, v220, s[20:21]"]
    for s in range(1, 8):
        body += ["v_cndmask_b32 v219, v%d, v220, %s" % (226 + s, masks[s]), "v_or_b32 v217, v217, v219"]
    assert findings(tmp_path, kernel(body)) == []


def test_a_vcc_write_at_the_end_of_a_loop_reaches_its_top_through_the_back_edge(tmp_path):
    loop = ["s_nop 4", ".Lloop_1:", "v_cndmask_b32 v3, v4, v5, vcc", "s_add_u32 s20, s20, 1", "s_cmp_lt_u32 s20, s21",
            "v_cmp_lt_i32 vcc, v1, v2", "s_cbranch_scc1 .Lloop_1"]
    bad = findings(tmp_path, kernel(loop))
    assert len(bad) == 1 and bad[0][2] == "valu-sgpr>valu" and bad[0][3] == 1      # only the s_cbranch stands between
    # the fall-through into the loop is clean: the region's leading s_nop 4 covers the compiler's vcc
    fixed = loop[:-1] + ["s_nop 0", "s_cbranch_scc1 .Lloop_1"]
    assert findings(tmp_path, kernel(fixed)) == []


def test_branches_to_labels_are_followed(tmp_path):
    """the replay's rare-path shape: a branch out of the loop body, a compare there, a branch back to a label right above a
    reader.  The fall-through path is padded, the branch path is not: flagged; padded on both: clean."""
    body = ["s_nop 4", "s_cbranch_scc1 .Lrare_1", "v_mov_b32 v9, 0", "s_nop 4", ".Lback_1:", "v_cndmask_b32 v3, v4, v5, vcc",
            "s_branch .Ldone_1", ".Lrare_1:", "v_cmp_gt_i32 vcc, s4, v1", "s_branch .Lback_1", ".Ldone_1:", "s_nop 0"]
    bad = findings(tmp_path, kernel(body))
    assert len(bad) == 1 and bad[0][2] == "valu-sgpr>valu" and bad[0][3] == 1
    fixed = body[:9] + ["s_nop 0"] + body[9:]
    assert findings(tmp_path, kernel(fixed)) == []


def test_region_entry_assumes_a_fresh_valu_write_of_every_input(tmp_path):
    """an asm statement cannot know what the compiler put in front of it: without its leading s_nop, a DPP read of an input
    register is flagged even when the compiler's code before the region writes nothing"""
    dpp = "v_add_u32_dpp v1, v1, v1 row_shr:1 row_mask:0xf bank_mask:0xf"
    bad = findings(tmp_path, kernel([dpp]))
    assert {f[2] for f in bad} == {"valu-vgpr>dpp", "trans>valu"} and all(f[1] is None for f in bad)    # (it may be a v_rcp)
    assert findings(tmp_path, kernel(["s_nop 1", dpp])) == []
    # a register the region wrote itself is not an input: no assumption about it, only the region's own producer counts
    assert findings(tmp_path, kernel(["v_mov_b32 v1, 0", "s_nop 1", dpp])) == []
    assert findings(tmp_path, kernel(["s_mov_b32 s10, 0", "v_add_u32 v2, s10, v3"])) == []
    assert [f[2] for f in findings(tmp_path, kernel(["s_nop 0", "v_add_u32 v2, s10, v3"]))] == ["valu-sgpr>valu"]


def test_compiler_code_is_out_of_scope_by_default_and_in_scope_for_the_calibration(tmp_path):
    text = "_Z4kernv:\n\tv_cmp_lt_i32 vcc, v1, v2\n\tv_cndmask_b32 v3, v4, v5, vcc\n\ts_endpgm\n"
    assert findings(tmp_path, text) == []
    assert [f[2] for f in findings(tmp_path, text, "--outside")] == ["valu-sgpr>valu"]


def built():
    files = sorted(glob.glob(os.path.join(OBJ, "*-hip-amdgcn-amd-amdhsa-gfx950.s")))
    if not files:
        pytest.skip("no compiler assembly under csrc/obj (library built elsewhere)")
    return files


def test_shipped_build_has_no_hazard_in_its_asm_regions():
    """every asm region of every kernel: both generated loops of the K = 8 kernel in all their instantiations, the DPP scan
    macros of gibbs_device.hpp, and whatever is added later"""
    files = built()
    assert len(files) >= 10
    assert sum(open(f).read().count(";;#ASMSTART") for f in files) > 1000
    r = subprocess.run([sys.executable, TOOL] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "0 finding(s)" in r.stdout


def test_rule_table_is_calibrated_on_the_compilers_own_code():
    """hipcc pads its own code correctly: the same rule table over the compiler's code (both ends of a pair outside every asm
    region) must find nothing, or the table (or the walk) is wrong"""
    r = subprocess.run([sys.executable, TOOL, "--outside"] + built(), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
