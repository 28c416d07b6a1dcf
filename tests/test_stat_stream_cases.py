"""The contract of the statistic device entries' shared test module, checked without a GPU: tests/stat_device_entry.py has a row
for every hmcg_*_device symbol the built library exports beside the sampler's own entry -- a tenth statistic cannot join without
the stream tests of tests/test_gpu_stat_streams.py --, each row's launch count is the one its stat_device(...) call passes in
csrc/hmcg.hip, and the cases of the stream tests are what they were chosen to be: `large` exceeds `small` in windows and in
slabs for every feature, every case has from its *_cases module alone a finite reference and a positive bound, and the
long-double score reference stays inside score_cases.PAIR_BUDGET."""
import os
import re

import numpy as np
import pytest

import kernel_tables as kt
import score_cases as sc
import stat_device_entry as sde
from hmc_jl_amd import _lib

SAMPLER_ENTRY = "hmcg_estimate_batch_device"
FEATURES = tuple(sde.FEATURES)


def test_every_exported_device_entry_has_a_row():
    exported = kt.library_symbols(r"hmcg_\w+_device") - {SAMPLER_ENTRY}
    declared = {n for n in _lib.EXPORTS + _lib.ORDER_EXPORTS + _lib.ERGODIC_EXPORTS + _lib.FAN_EXPORTS + _lib.SCORE_EXPORTS if n.endswith("_device")}
    assert exported == declared - {SAMPLER_ENTRY}, (sorted(exported), sorted(declared))
    rows = {sde.entry_symbol(f): f for f in FEATURES}
    assert len(rows) == len(FEATURES) == 9
    assert set(rows) == exported, (sorted(set(rows) ^ exported))
    for f in FEATURES:
        assert callable(getattr(_lib, sde.FEATURES[f].call))


def source_launches():
    """{exported symbol: the launches expression its stat_device(...) call passes}, parsed from csrc/hmcg.hip: the export's body
    names the feature's device function, whose body holds the one stat_device call."""
    text = kt._code(os.path.join(kt.CSRC, "hmcg.hip"))
    frames = {}
    for m in re.finditer(r"\nint (\w+_device)\(DeviceCtx& c,", text):
        call = re.search(r"stat_device\(c, .*?timing, (?:\{[^}]*\}|\w+\(\w*\)), (.+?), \[&\]\(\) -> int \{", text[m.end():], re.S)
        nxt = re.search(r"\nint \w+\(", text[m.end():])
        if call and (nxt is None or call.start() < nxt.start()):                  # (launch_device, the sampler's, has none)
            frames[m.group(1)] = call.group(1).strip()
    assert len(frames) == text.count("return stat_device(") == 9, sorted(frames)
    out = {}
    for m in re.finditer(r"\nint (hmcg_\w+_device)\(", text):
        inner = re.search(r"return (\w+_device)\(c, p", text[m.end():])
        if m.group(1) != SAMPLER_ENTRY:
            out[m.group(1)] = frames[inner.group(1)]
    return out


def c_int(expr, **names):
    """A launches expression of hmcg.hip as a number: an integer expression over `names`, or `flag ? a : b`."""
    m = re.fullmatch(r"(\w+) \? (.+) : (.+)", expr)
    if m:
        return c_int(m.group(2) if names[m.group(1)] else m.group(3), **names)
    assert re.fullmatch(r"[\w\s+*()]+", expr), expr
    return int(eval(expr, {"__builtins__": {}}, names))


def test_rows_report_the_launches_of_the_source():
    src = source_launches()
    assert set(src) == {sde.entry_symbol(f) for f in FEATURES}
    seen = set()
    for f in FEATURES:
        row, expr = sde.FEATURES[f], src[sde.entry_symbol(f)]
        case = sde.stream_case(f, "small")
        variants = [case]
        if "lo_hi" in case:
            variants.append(dict(case, lo_hi=np.zeros(case["x"].shape[:2] + (2,))))
        if "rounds" in case:
            variants += [dict(case, rounds=r) for r in (0, 2, _lib.FAN_MAXROUNDS)]
        for c in variants:
            names = {"dlo_hi": c.get("lo_hi") is not None, "R": sde.fc.rounds_of(c["rounds"]) if "rounds" in c else None}
            assert row.launches(c) == c_int(expr, **names), (f, expr)
            seen.add((f, row.launches(c)))
    assert {n for f, n in seen if f == "chain_density"} == {3, 4} and len({n for f, n in seen if f == "predictive_quantiles"}) == 4


@pytest.mark.parametrize("feature", FEATURES)
def test_large_exceeds_small_in_windows_and_slabs(feature):
    assert _lib.PRED_SLAB == 1024
    slabs = lambda nd: -(-nd // _lib.PRED_SLAB)
    small, large, again = (sde.stream_case(feature, s) for s in ("small", "large", "small2"))
    first = lambda c: c["x"] if "x" in c else c["mu"]
    assert first(large).shape[0] > first(small).shape[0] and slabs(large["nd"]) >= 3 > slabs(small["nd"]) == 1
    assert first(small).shape == first(again).shape and not np.array_equal(first(small), first(again))
    assert first(small).shape[1] == sde.K == 3 and large["nd"] % 64 and small["nd"] % 64
    if "horizons" in small or "hz" in small:
        assert max(small.get("horizons", small.get("hz"))) > 0 and small["A"] is not None          # A is read


@pytest.mark.parametrize("shape", ["small", "large"])
@pytest.mark.parametrize("feature", FEATURES)
def test_stream_cases_have_a_finite_reference_and_a_positive_bound(feature, shape):
    row = sde.FEATURES[feature]
    case = sde.stream_case(feature, shape)
    refs, bounds = row.judged(case, row.reference(case))
    assert refs
    for r in refs:
        assert np.isfinite(np.asarray(r, dtype=np.float64)).all(), (feature, shape)
    for b in bounds:
        b = np.asarray(b, dtype=np.float64)
        assert np.isfinite(b).all() and (b > 0.0).all(), (feature, shape)
    assert bounds or feature == "chain_quantiles"             # a selection is compared bit for bit


def test_score_cases_stay_inside_the_pair_budget():
    for shape, (W, nd, _) in sde.SHAPES.items():
        case = sde.stream_case("predictive_scores", shape)
        stride, n_u = sc.thinning(nd, case["stride"])
        assert stride == sde.SCORE_STRIDE and sc.pair_cost(sde.K, n_u, W) <= sc.PAIR_BUDGET, shape
    assert sc.thinning(sde.SHAPES["large"][1], sde.SCORE_STRIDE)[1] * sde.K > 2 * 2 * sc.TP          # more than two blocks of the pair pass
