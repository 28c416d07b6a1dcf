"""`tools/isa_bytes.py`: code bytes of a kernel, its loops' address ranges and its barriers' addresses, on a hand-made
kernel whose encodings are known (4-byte SOP, 8-byte VOP3).  No GPU: the tool assembles with the ROCm llvm-mc."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "isa_bytes.py")
LLVM_MC = os.path.join(os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin"), "llvm-mc")

KERNEL = """\t.text
\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"
\t.section\t.text._Z1kv,"axG",@progbits,_Z1kv,comdat
\t.protected\t_Z1kv
\t.globl\t_Z1kv
\t.p2align\t8
\t.type\t_Z1kv,@function
_Z1kv:
\ts_mov_b32 s0, 0
.LBB0_1:
\ts_add_u32 s0, s0, 1
\tv_add_f64 v[0:1], v[0:1], v[0:1]
\ts_barrier
\ts_cmp_lt_u32 s0, 10
\ts_cbranch_scc1 .LBB0_1
\ts_endpgm
.Lfunc_end0:
\t.size\t_Z1kv, .Lfunc_end0-_Z1kv
"""


def test_bytes_of_a_known_kernel(tmp_path):
    if not os.path.exists(LLVM_MC):
        pytest.skip("no llvm-mc under the ROCm tree")
    s = tmp_path / "k.s"
    s.write_text(KERNEL)
    r = subprocess.run([sys.executable, TOOL, str(s), "k()", "--min", "0"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert out[0] == "k()" and out[1].startswith("kernel: 32 bytes (1 lines"), out[:2]
    loop = [ln.split() for ln in out if ln.startswith(".LBB0_1")]
    assert loop == [[".LBB0_1", "4", "5", "12"]], loop          # starts behind the s_mov; five instructions; label -> the barrier's label
    assert out[-2].endswith(": 0+16") or out[-1].endswith(": 0+16"), out[-2:]      # s_mov, s_add: 4 each; v_add_f64: 8
