"""What the library compiles, read from its sources: the one parser of csrc/variants.hpp and csrc/variants_*.hip and what
follows from it -- the register-resident ladder of every (K, path), the instantiations of the LDS-resident kernel, the lengths
that reach them.  A plain module for the test modules and their case tables; importing it needs no GPU, no numpy and no load
of the library.  tests/test_variant_coverage.py holds the parse to the kernel symbols of the built libhmcgibbs.so, so a regex
that silently drops a row fails there.

csrc/variants.hpp (HMCG_BIG_FORM: the K list) and the variants_big*.hip units (g_big_xyz = HMCG_BIG_FORM(sig, smooth, stream))
define 8 forms x K = 2..8 = 56 separately compiled LDS-resident kernels; the variants_*.hip tables hold the register-resident
rows: HMCG_V3(K, L, sig, smooth, ...) expands to three flavours, HMCG_V(K, L, NT, sig, smooth, NH, OCC, ...) is one kernel.  A
new unit, row, K or form is picked up by everything derived here.

Below that, what the two per-instantiation contracts share (test_variant_coverage.py for the sampler, test_stat_coverage.py for
the draw-statistic kernels): a test's parametrize list, the kernel symbols of the built library (read with nm from the file, not
by loading it), and the launch rules of the statistic units parsed from their sources."""
import glob
import os
import re
import shutil
import subprocess

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


# ---- what the per-instantiation contracts share (tests/test_variant_coverage.py, tests/test_stat_coverage.py) ----
def cases_of(test, argnames=None):
    """The argument tuples of a test function's pytest.mark.parametrize: what the suite actually runs.  A test with several
    parametrize marks names the one it means by its argnames."""
    marks = [m for m in getattr(test, "pytestmark", []) if m.name == "parametrize" and (argnames is None or m.args[0] == argnames)]
    assert len(marks) == 1, test.__name__
    return list(marks[0].args[1])


def library_symbols(pattern):
    """The defined dynamic symbols of the built libhmcgibbs.so that match `pattern` (a regex over one symbol name), as a set.
    Read with nm from the file: the library is not loaded."""
    from hmc_jl_amd import _lib
    nm = shutil.which("nm") or shutil.which("llvm-nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    assert nm, "no nm / llvm-nm to list the symbols of libhmcgibbs.so"
    assert os.path.exists(_lib.SO_PATH), "libhmcgibbs.so is not built"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.SO_PATH], check=True, capture_output=True, text=True).stdout
    return set(re.findall(r"\b(%s)\b" % pattern, out))


def template_ints(field):
    """The integer template arguments of an Itanium name's I...E field: its Li<int>E / Lb<0|1>E entries, in order."""
    return [int(x) for x in re.findall(r"L[ib](\d+)E", field)]


# The templated draw-statistic kernels: name -> (unit that launches it, number of integer template arguments).
STAT_KERNELS = {
    "predictive_cdf_kernel": ("predictive.hip", 1),
    "fan_eval_kernel": ("fan.hip", 1),
    "score_comp_kernel": ("score.hip", 1),
    "score_pair_kernel": ("score.hip", 1),
    "mixmoments_kernel": ("mixmoments.hip", 2),
    "bias_moments_kernel": ("bias.hip", 1),
    "ergodic_kernel": ("ergodic.hip", 1),
    "draw_moments_kernel": ("moments.hip", 1),
}


def stat_instantiations():
    """{kernel name: sorted list of template-argument tuples} of the draw-statistic kernels in the built library, from the kernel
    handles of its dynamic symbol table (_ZN4hmcg<len><name>I<Li..E>+EEvNS_<len><Params>E; the __device_stub__ twins are other
    names).  A handle of one of these kernels whose shape the pattern does not know fails here."""
    names = library_symbols(r"_ZN4hmcg\d+(?:%s)I\w+" % "|".join(STAT_KERNELS))
    out = {k: [] for k in STAT_KERNELS}
    for name in sorted(names):
        m = re.match(r"_ZN4hmcg(\d+)([a-z_]+)I((?:L[ib]\d+E)+)EEvNS_\d+\w+ParamsE$", name)
        assert m and m.group(2) in STAT_KERNELS and int(m.group(1)) == len(m.group(2)), "kernel symbol of an unknown shape: " + name
        args = tuple(template_ints(m.group(3)))
        assert len(args) == STAT_KERNELS[m.group(2)][1], name
        out[m.group(2)].append(args)
    return {k: sorted(v) for k, v in out.items()}


def switch_cases(text, selector, launch):
    """{case value: launched template argument} of `switch (<selector>) { case n: <launch>(m); break; ... }` in a source text
    without comments; the whole body up to the closing brace must consist of such lines (and a default)."""
    m = re.search(r"switch\s*\(\s*%s\s*\)\s*\{(.*?)\}" % re.escape(selector), text, re.S)
    assert m, "no switch (%s)" % selector
    body = m.group(1).replace("\\\n", "\n")
    rows = re.findall(r"case\s+(\d+)\s*:\s*%s\(\s*(\d+)\s*\)\s*;\s*break\s*;" % re.escape(launch), body)
    rest = re.sub(r"case\s+\d+\s*:\s*%s\(\s*\d+\s*\)\s*;\s*break\s*;" % re.escape(launch), "", body)
    rest = re.sub(r"default\s*:[^;]*;", "", rest).strip()
    assert rows and not rest, "switch (%s): lines of another shape: %r" % (selector, rest)
    out = {int(a): int(b) for a, b in rows}
    assert len(out) == len(rows), "switch (%s): a case twice" % selector
    return out


def header_int(name, path=os.path.join(ROOT, "include", "hmcg.h")):
    """#define <name> <int> of a header."""
    m = re.search(r"^\s*#\s*define\s+%s\s+(\d+)\b" % name, open(path).read(), re.M)
    assert m, name
    return int(m.group(1))


def stat_switch_k():
    """HMCG_SWITCH_K of csrc/stat_device.hpp: {K: the K_ it launches}."""
    text = _code(os.path.join(CSRC, "stat_device.hpp")).replace("\\\n", "\n")
    m = re.search(r"#define\s+HMCG_SWITCH_K\(k_,\s*LAUNCH_\)\s*(switch.*?\})", text, re.S)
    assert m, "HMCG_SWITCH_K"
    return switch_cases(m.group(1), "k_", "LAUNCH_")


def stat_launch_rules():
    """How each draw-statistic unit picks its instantiation, parsed from the launch lines of its source (comments removed):
      'K'     {K: K_}: HMCG_SWITCH_K, and that predictive / fan / score / mixmoments / bias / ergodic launch through it on a.K with
              a macro whose kernel takes K_ first;
      'pair'  {n_h: NH} of score.hip's switch (a.n_h);
      'nhc'   (limit, small, large): mixmoments.hip launches <K_, small> if a.n_h <= limit, else <K_, large> (HMCG_MAXH resolved
              from include/hmcg.h)."""
    by_k = stat_switch_k()
    for unit, kernel, macro in (("predictive.hip", "predictive_cdf_kernel", "HMCG_PRED"), ("fan.hip", "fan_eval_kernel", "HMCG_FAN_EVAL"),
                                ("score.hip", "score_comp_kernel", "HMCG_SCORE_COMP"), ("mixmoments.hip", "mixmoments_kernel", "HMCG_MIX"),
                                ("bias.hip", "bias_moments_kernel", "HMCG_BIAS"), ("ergodic.hip", "ergodic_kernel", "HMCG_ERG")):
        text = _code(os.path.join(CSRC, unit))
        assert re.search(r"HMCG_SWITCH_K\(\s*a\.K\s*,\s*%s\s*\)" % macro, text), (unit, "does not launch through HMCG_SWITCH_K(a.K, %s)" % macro)
        d = re.search(r"#define\s+%s\(K_\)((?:[^\n]*\\\n)*[^\n]*)" % macro, text)
        assert d, (unit, macro)
        used = re.findall(r"hmcg::(\w+)<([^>]*)>", d.group(1))
        assert used and all(k == kernel and a.split(",")[0].strip() == "K_" for k, a in used), (unit, used)
    score = _code(os.path.join(CSRC, "score.hip"))
    assert re.search(r"#define\s+HMCG_SCORE_PAIR\(NH_\)\s+hipLaunchKernelGGL\(\s*hmcg::score_pair_kernel<NH_>", score)
    pair = switch_cases(score, "a.n_h", "HMCG_SCORE_PAIR")
    mix = _code(os.path.join(CSRC, "mixmoments.hip")).replace("\\\n", "\n")
    m = re.search(r"if\s*\(\s*a\.n_h\s*<=\s*(\d+)\s*\)\s*hipLaunchKernelGGL\(\(hmcg::mixmoments_kernel<K_,\s*(\w+)>\)[^;]*;\s*"
                  r"else\s+hipLaunchKernelGGL\(\(hmcg::mixmoments_kernel<K_,\s*(\w+)>\)", mix)
    assert m, "mixmoments.hip: the two launch lines of HMCG_MIX"
    val = lambda s: int(s) if s.isdigit() else header_int(s)
    return {"K": by_k, "pair": pair, "nhc": (int(m.group(1)), val(m.group(2)), val(m.group(3)))}


def bias_constants():
    """What csrc/bias.hip deals its items by, read from its source: 'waves' = BIAS_NT / 64, 'items' = bias_nitems as a function
    of K (the constexpr one-liners bias_nv / bias_nc / bias_np / bias_nitems, evaluated as written), 'unroll_max' = the largest
    K whose four sub-tiles are unrolled (UNR = K <= n ? BIAS_NW : 1)."""
    text = _code(os.path.join(CSRC, "bias.hip"))
    nt = int(re.search(r"constexpr\s+int\s+BIAS_NT\s*=\s*(\d+)\s*;", text).group(1))
    assert re.search(r"constexpr\s+int\s+BIAS_NW\s*=\s*BIAS_NT\s*/\s*64\s*;", text)
    fns = dict(re.findall(r"constexpr\s+int\s+(bias_n\w+)\(int K\)\s*\{\s*return\s+([^;]+);\s*\}", text))
    assert set(fns) >= {"bias_nv", "bias_nc", "bias_np", "bias_nitems"}, sorted(fns)
    assert all(re.fullmatch(r"[\w\s()+*]+", body) for body in fns.values()), fns      # sums and products of K and each other

    def call(name, K):
        env = {n: (lambda k, n=n: call(n, k)) for n in fns}
        env["K"] = K
        return eval(fns[name], {"__builtins__": {}}, env)
    m = re.search(r"UNR\s*=\s*K\s*<=\s*(\d+)\s*\?\s*BIAS_NW\s*:\s*1\b", text)
    assert m, "bias.hip: the unroll switch"
    assert re.search(r"PPW\s*=\s*\(bias_nitems\(K\)\s*\+\s*BIAS_NW\s*-\s*1\)\s*/\s*BIAS_NW", text)
    return {"waves": nt // 64, "items": lambda K: call("bias_nitems", K), "unroll_max": int(m.group(1))}
