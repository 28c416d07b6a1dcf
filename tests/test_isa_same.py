"""`tools/isa_same.py`: the text comparison of two builds' device assembly behind the rule of DESIGN.md section 9 (a
refactor of the kernels is done when every shipped kernel's machine code is unchanged).  Hand-made snippets: what
cannot reach the GPU (comments, trailing blanks, debug-line directives) is ignored, everything else counts."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = "variants_k3-hip-amdgcn-amd-amdhsa-gfx950.s"
K1 = "_ZN4hmcg19gibbs_sweeps_kernelILi3ELi4ELi256ELb0ELb0ELi4ELi2EEEvNS_12KernelParamsE"
K2 = "_ZN4hmcg19gibbs_sweeps_kernelILi3ELi8ELi256ELb0ELb0ELi0ELi1EEEvNS_12KernelParamsE"


def kernel(name, n):
    return """\
\t.globl\t%(k)s
\t.p2align\t8
\t.type\t%(k)s,@function
%(k)s: ; @%(k)s
; %%bb.0:
\ts_load_dwordx2 s[2:3], s[0:1], 0x0
\tv_writelane_b32 v191, s6, 0
\tv_add_f64 v[10:11], v[4:5], v[6:7]
.LBB%(n)d_1: ; %%Flow2790
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel %(k)s
\t\t.amdhsa_next_free_vgpr 192
\t\t.amdhsa_next_free_sgpr 96
\t.end_amdhsa_kernel
\t.text
""" % {"k": name, "n": n}


def meta(name, sspill):
    return """\
  - .agpr_count:     0
    .args:
      - .offset:         0
        .size:           8
    .group_segment_fixed_size: 28480
    .name:           %s
    .private_segment_fixed_size: 0
    .sgpr_spill_count: %d
    .vgpr_count:     192
    .vgpr_spill_count: 0
""" % (name, sspill)


def asm(k1=None, k2=None, m1=113, m2=52):
    return ("\t.text\n\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"\n" + (k1 or kernel(K1, 0)) + (k2 or kernel(K2, 1))
            + "\t.amdgpu_metadata\n---\namdhsa.kernels:\n" + meta(K1, m1) + meta(K2, m2) + "amdhsa.version:\n  - 1\n...\n\t.end_amdgpu_metadata\n")


BASE = asm()


def compare(tmp_path, a, b):
    """isa_same on two object directories holding the given {file name: text}; (exit status, output)."""
    for side, files in (("a", a), ("b", b)):
        os.makedirs(tmp_path / side)
        for name, text in files.items():
            (tmp_path / side / name).write_text(text)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_same.py"), str(tmp_path / "a"), str(tmp_path / "b")],
                       capture_output=True, text=True)
    return r.returncode, r.stdout


def test_comments_blanks_and_debug_lines_do_not_count(tmp_path):
    other = BASE.replace("%Flow2790", "%Flow2788").replace("\ts_endpgm\n", "\t.loc\t1 1414 9 is_stmt 0\n\ts_endpgm  \t\n")
    other = other.replace("\t.text\n\t.amdgcn_target", "\t.text\n\t.file\t\"variants_k3.hip\"\n\t.cfi_sections .debug_frame\n\t.amdgcn_target", 1)
    other += "\t.ident\t\"clang\"\n; a trailing comment\n"
    assert other != BASE
    rc, out = compare(tmp_path, {UNIT: BASE}, {UNIT: other})
    assert rc == 0, out
    assert "variants_k3" in out and "identical" in out and "differs" not in out


def only_second_kernel_differs(tmp_path, other):
    rc, out = compare(tmp_path, {UNIT: BASE}, {UNIT: other})
    assert rc == 1, out
    assert "variants_k3" in out and "differs" in out
    assert "gibbs<3,8,256,0,0,0,1>" in out and "gibbs<3,4,256,0,0,4,2>" not in out, out


def test_a_register_number_counts(tmp_path):
    only_second_kernel_differs(tmp_path, asm(k2=kernel(K2, 1).replace("v191", "v193")))


def test_a_kernel_descriptor_field_counts(tmp_path):
    only_second_kernel_differs(tmp_path, asm(k2=kernel(K2, 1).replace(".amdhsa_next_free_sgpr 96", ".amdhsa_next_free_sgpr 98")))


def test_a_spill_count_in_the_metadata_counts(tmp_path):
    only_second_kernel_differs(tmp_path, asm(m2=54))


def test_a_unit_missing_on_one_side(tmp_path):
    big = "variants_big-hip-amdgcn-amd-amdhsa-gfx950.s"
    rc, out = compare(tmp_path, {UNIT: BASE, big: BASE}, {UNIT: BASE})
    assert rc == 1, out
    assert "variants_big" in out and "missing" in out
    assert [ln for ln in out.splitlines() if ln.startswith("variants_k3")][0].split()[1] == "identical"
