"""What the library compiles, read from its sources: the one parser of csrc/variants.hpp and csrc/variants_*.hip and what
follows from it -- the register-resident ladder of every (K, path), the instantiations of the LDS-resident kernel, the lengths
that reach them.  A plain module for the test modules and their case tables; importing it needs no GPU, no numpy and no load
of the library.  tests/test_variant_coverage.py holds the parse to the kernel symbols of the built libhmcgibbs.so, so a regex
that silently drops a row fails there.

csrc/variants.hpp (HMCG_BIG_FORM: the K list) and the variants_big*.hip units (g_big_xyz = HMCG_BIG_FORM(sig, smooth, stream))
define 8 forms x K = 2..8 = 56 separately compiled LDS-resident kernels; the variants_*.hip tables hold the register-resident
rows: HMCG_V3(K, L, sig, smooth, ...) expands to three flavours, HMCG_V(K, L, NT, sig, smooth, NH, OCC, ...) is one kernel.  A
new unit, row, K or form is picked up by everything derived here."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hmc.jl_amd", "csrc")
NT = 256
LDS_LIMIT = 160 * 1024                 # plan.hpp, choose_big: dynamic + static LDS of the instantiation must fit the CU's 160 KiB
FLAVOUR_WAVES = {"p1": (0, 1), "p2": (0, 2), "h": (4, 2)}        # HMCG_FLAVOUR -> (NH, OCC) of the three HMCG_V3 expansions: (helper_waves, occupancy)
PATH = {"base": (False, False), "sig": (True, False), "smooth": (False, True)}      # path -> (sig, smooth)


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


def register_classes(K, sig, smooth):
    """The steps-per-thread classes of the 256-thread register-resident rows of (K, path), ascending."""
    return sorted({L for (k, L, nt, s, m, _, _) in REG_ROWS if (k, nt, s, m) == (K, NT, sig, smooth)})


def ladder_ceiling(K, sig, smooth):
    """The longest window the register-resident kernels of (K, path) hold at 256 threads per window (0: there are none)."""
    return max([NT * L for (k, L, nt, s, m, _, _) in REG_ROWS if (k, nt, s, m) == (K, NT, sig, smooth)], default=0)


def steps_per_thread(K, T, sig=False, smooth=False):
    """The class the dispatch gives a window of T steps: the smallest 256-thread class of (K, path) with 256 L >= T."""
    return min(L for L in register_classes(K, sig, smooth) if NT * L >= T)


def variant_rows():
    """(K, L, path) of the HMCG_V3 rows: the rows of REG_ROWS that exist in the helper flavour, which HMCG_V3 alone expands to."""
    name = {v: k for k, v in PATH.items()}
    return [(K, L, name[sig, sm]) for (K, L, nt, sig, sm, nh, occ) in REG_ROWS if (nh, occ) == FLAVOUR_WAVES["h"]]


VARIANT_ROWS = variant_rows()
VARIANT_CASES = [(K, L, path, fl) for (K, L, path) in VARIANT_ROWS for fl in ("p1", "p2", "h")]
SIGSMOOTH = [(K, L) for (K, L, nt, sig, sm, _, _) in REG_ROWS if (nt, sig, sm) == (NT, True, True)]      # the SIG + SM rows: HMCG_V, plain flavour
OWN_THREAD_COUNT = [(K, L, nt) for (K, L, nt, _, _, _, _) in REG_ROWS if nt != NT]       # rows selected by threads_per_window=NT

STREAM_T = NT * ((LDS_LIMIT - 16) // (NT * 21) + 1) - 1         # 7935: beyond the LDS even with no static share at all


def coverage_lengths(sig, smooth, stream, K):
    """Window lengths of the coverage case of one LDS-resident instantiation (longest first): beyond the register-resident
    ladder of its (K, path) and no multiple of 256 -- beyond the LDS for a streaming form --, then short windows, which make_plan
    leaves on the same launch."""
    top = STREAM_T if stream else max(ladder_ceiling(K, sig, smooth), 2 * NT) + NT + 45
    return [top, 8 if sig else 2, 64, 65, 257]
