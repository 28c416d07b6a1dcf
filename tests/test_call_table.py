"""The table of a call's buffers (_lib.BUFFERS, call_dims, build_call) and the two runners on top of it, checked without a GPU:
the table against include/hmcg.h; the host runner (estimate_batch_host over a library stand-in that records its arguments)
against the device runner (tests/device_entry.py over placeholder addresses) on every device-entry parity case and a grid of
host requests, where they may differ by exactly what build_call documents; the name lists derived from the table; and
DevicePanel's shapes."""
import ctypes as C
import types

import numpy as np
import pytest

import device_entry as de
import hmcg_header
import test_gpu_device_entry as dev
from hmc_jl_amd import _lib, device

ROWS = {r.name: r for r in _lib.BUFFERS}
C_TYPE = {"double": np.float64, "int32_t": np.int32, "uint32_t": np.uint32, "uint8_t": np.uint8}
# how include/hmcg.h spells a dimension -> the symbol of call_dims
HEADER_DIM = {"n_samples": "ns", "nsave_ld": "nsave", "3K+K*K+2H": "NS", "3K+K*K+2H+K": "NS+K"}


# ---- the table against the header ----
def test_one_row_per_array_of_the_header():
    names = [r.name for r in _lib.BUFFERS]
    assert len(set(names)) == len(names), "a name has two rows"
    params = hmcg_header.entry_data_pointers("hmcg_estimate_batch")
    assert [(r.name, r.pos) for r in _lib.BUFFERS if r.pos is not None] == [(name, i) for i, (name, _, _) in enumerate(params)]
    # (the device and the multi-device entries take the same arrays in the same order)
    assert [p[0][1:] for p in hmcg_header.entry_data_pointers("hmcg_estimate_batch_device") if p[0] != "stream"] == [p[0] for p in params]
    assert hmcg_header.entry_data_pointers("hmcg_estimate_batch_multi")[1:] == params
    # (the header's opening comment: Y window-major with leading dimension ldY, yreal Julia (H, W))
    assert [ROWS[n].shape for n in ("Y", "T", "yreal")] == [("W", "ldY"), ("W",), ("W", "H")]
    members = hmcg_header.extras_pointers()
    assert sorted(r.name for r in _lib.BUFFERS if r.pos is None) == sorted(members)      # none missing, none the header lacks
    for name, ctype, const in params:
        assert (ROWS[name].dtype, ROWS[name].io) == (C_TYPE[ctype], "in" if const else "out"), name
    for name, (ctype, const, layout) in members.items():
        assert (ROWS[name].dtype, ROWS[name].io) == (C_TYPE[ctype], "in" if const else "out"), name
        assert list(ROWS[name].shape) == [HEADER_DIM.get(d, d) for d in layout], name


def test_dimension_symbols():
    sr = np.array([[3, 9], [0, 2], [5, 5]], dtype=np.int32)
    d = _lib.call_dims(3, 50, 4, 6, 2, n_samples=5, save_range=sr)
    assert d == {"W": 3, "ldY": 50, "K": 4, "H": 2, "2H": 4, "NS": 32, "NS+K": 36, "NC": 29, "ns": 5, "nd": 30, "nsave": 6, "2": 2}
    d = _lib.call_dims(3, 50, 2, 6, 0)
    assert (d["ns"], d["nd"], d["NS"], d["NC"], d["nsave"]) == (1, 6, 10, 11, 0)
    assert _lib.call_dims(1, 9, 2, 6, 0, save_range=np.array([[4, 4]]))["nsave"] == 1
    assert {s for r in _lib.BUFFERS for s in r.shape} <= set(d)


# ---- the host runner against the device runner ----
class RecordingLibrary:
    """Stands in for libhmcgibbs.so under estimate_batch_host: keeps what the entry was called with, computes nothing."""

    def hmcg_estimate_batch(self, cfg, *a):
        self.cfg, self.args, self.extras, self.devices = cfg._obj, a[:10], a[10]._obj, None
        return 0

    def hmcg_estimate_batch_multi(self, cfg, n, devs, *a):
        self.cfg, self.args, self.extras, self.devices = cfg._obj, a[:10], a[10]._obj, list(devs)
        assert n.value == len(devs) == len(a[11])
        return 0


@pytest.fixture
def library(monkeypatch):
    monkeypatch.setattr(_lib, "_LIB", RecordingLibrary())
    return _lib._LIB


def members_set(ex):
    return {n for n, t in _lib.Extras._fields_ if t is C.c_void_p and getattr(ex, n)}


def host_call(library, args, kw):
    """(the hmcg_extras members passed, {buffer: shape}, the result, hmcg_config's bytes) of estimate_batch_host(*args, **kw);
    every pointer the entry received is the array of that name in the result, or an input."""
    out = _lib.estimate_batch_host(*args, **kw)
    arrays = {k: v for k, v in out.items() if isinstance(v, np.ndarray)}
    passed = {n: p.value for n, p in zip([r.name for r in _lib.BUFFERS if r.pos is not None], library.args) if p is not None}
    passed.update({n: getattr(library.extras, n) for n in members_set(library.extras)})
    assert {n for n in passed if ROWS[n].io == "out"} == set(arrays)
    for n, v in arrays.items():
        assert passed[n] == v.ctypes.data and v.flags.c_contiguous and v.dtype == ROWS[n].dtype, n
    return members_set(library.extras), {k: v.shape for k, v in arrays.items()}, out, bytes(library.cfg)


HOST_ONLY = ("want_draws", "devices", "out", "nan_fill", "resume_sample_summary")


def device_call(args, kw):
    c = de._build(de.PlaceholderCall(), *args, **{k: v for k, v in kw.items() if k not in HOST_ONLY})
    cfg, ptrs, ex = c.launch
    at = {t.data_ptr(): k for k, t in c.buf.items()}
    assert [at.get(p) for p in ptrs[3:]] == [r.name for r in _lib.BUFFERS if r.pos is not None and r.io == "out"]
    assert members_set(ex) == de.extras_passed(*args, **{k: v for k, v in kw.items() if k not in HOST_ONLY})
    return members_set(ex), {k: tuple(t.shape) for k, t in c.buf.items()}, ex, bytes(cfg)


@pytest.mark.parametrize("c", dev.PARITY_CASES, ids=[c["id"] for c in dev.PARITY_CASES])
def test_parity_cases_issue_the_same_call_on_both_entries(library, c):
    """What test_device_entry_against_oracle compares bit for bit are the same call: the same hmcg_extras members, buffers of
    the same shapes, and the same hmcg_config but for the min_T hint of the bucketed cases."""
    args, kw = dev.call_of(c)
    h_members, h_shapes, _, h_cfg = host_call(library, args, kw)
    d_members, d_shapes, _, d_cfg = device_call(args, dict(kw, **dev.device_kw(c)))
    assert h_members == d_members == dev.case_extras(c)
    assert h_shapes == d_shapes
    assert (h_cfg == d_cfg) == (not c["bucketed"])
    assert h_cfg == device_call(args, kw)[3]


W, LDY, K = 3, 24, 3
Y, TW = np.zeros((W, LDY)), np.array([24, 20, 9])
ARGS = (Y, TW, K, 2, 4, (12,), np.zeros((W, 1)))
SIG = np.stack([TW - 6, TW], axis=1)
SAVE = np.stack([TW - 5, TW - np.arange(W)], axis=1)                 # the longest: 5, 4, 3 positions -> nsave_ld 5
SIGNAL = dict(sig_range=SIG, save_range=SAVE, sigma_signal=[0.4, 1.3, 0.05], end_pos=TW - 3, kappa=0.6, n_samples=3)
STATE = dict(status=np.full(W, 8, np.int32), xstate=np.ones((W, LDY), np.uint8), sumacc=np.full((W, 3 * K + K * K + 2 + K), 0.5))
DRAWS = {"mu", "sig2", "A", "pi_end", "fcast"}
# (id, keywords, what the device runner alone passes and allocates, what it alone allocates): the documented differences --
# pif_final with a smoothing output and no want_state; every draw array whatever want_draws says
GRID = [
    ("base", {}, set(), set()),
    ("want_state", dict(want_state=True), set(), set()),
    ("want_draws-false", dict(want_draws=False), set(), DRAWS),
    ("want_draws-subset", dict(want_draws=("mu", "fcast")), set(), {"sig2", "A", "pi_end"}),
    ("x_init", dict(x_init=np.zeros((W, LDY))), set(), set()),
    ("window_ids", dict(window_ids=[7, 3, 11]), set(), set()),
    ("signal", SIGNAL, set(), set()),
    ("signal-no-save_range", {k: v for k, v in SIGNAL.items() if k != "save_range"}, set(), set()),
    ("signal-no-sigma_signal", {k: v for k, v in SIGNAL.items() if k != "sigma_signal"}, set(), set()),
    ("signal-no-end_pos", {k: v for k, v in SIGNAL.items() if k != "end_pos"}, set(), set()),
    ("signal-blend_mask", dict(SIGNAL, blend_mask=1), set(), set()),
    ("signal-n_samples-0", dict(SIGNAL, n_samples=0), set(), set()),
    ("signal-n_samples-1", dict(SIGNAL, n_samples=1), set(), set()),
    ("signal-inputs-without-sig_range", {k: v for k, v in SIGNAL.items() if k != "sig_range"}, set(), set()),
    ("sample_summary", dict(SIGNAL, want_sample_summary=True), set(), set()),
    ("sample_summary-resumed", dict(SIGNAL, want_sample_summary=True, resume_state=dict(STATE, sample_summary=np.ones((W, 3, 20))),
                                    resume_sample_summary=np.ones((W, 3, 20)), sweep_base=8), set(), set()),
    ("want_smooth", dict(want_smooth=True), {"pif_final"}, set()),
    ("want_filter_mean", dict(want_filter_mean=True), {"pif_final"}, set()),
    ("want_smooth_draws", dict(want_smooth_draws=True), {"pif_final"}, set()),
    ("smoothing-together", dict(want_smooth=True, want_filter_mean=True, want_smooth_draws=True), {"pif_final"}, set()),
    ("smoothing-with-state", dict(want_smooth=True, want_filter_mean=True, want_smooth_draws=True, want_state=True), set(), set()),
    ("want_corr", dict(want_corr=True), set(), set()),
    ("want_corr-no-draws", dict(want_corr=True, want_draws=False), set(), DRAWS),
    ("resumed", dict(resume_state=STATE, sweep_base=3, sweep_count=2), set(), set()),
    ("devices-0", dict(devices=[0]), set(), set()),
    ("devices-0-1", dict(devices=[0, 1], want_state=True), set(), set()),
]


@pytest.mark.parametrize("id,kw,device_only_members,device_only_draws", GRID, ids=[g[0] for g in GRID])
def test_host_grid_issues_the_same_call_on_both_entries(library, id, kw, device_only_members, device_only_draws):
    h_members, h_shapes, out, h_cfg = host_call(library, ARGS, kw)
    d_members, d_shapes, ex, d_cfg = device_call(ARGS, kw)
    assert h_members <= d_members and d_members - h_members == device_only_members
    assert set(h_shapes) <= set(d_shapes) and set(d_shapes) - set(h_shapes) == device_only_members | device_only_draws
    assert h_shapes == {k: d_shapes[k] for k in h_shapes}
    assert h_cfg == d_cfg and library.extras.nsave_ld == ex.nsave_ld
    assert library.devices == kw.get("devices")
    assert bool(library.cfg.flags & _lib.FLAG_RESUME) == ("resume_state" in kw)
    if "sig_range" in kw and "save_range" in kw:
        assert ex.nsave_ld == 5 and h_shapes["sigvals"] == (W, max(kw["n_samples"], 1), 5)
    else:
        assert ex.nsave_ld == 0 and "sigvals" not in d_shapes
    if "sig_range" not in kw:                                # both runners ignore the signal-path inputs then
        assert not {"save_range", "sigma_signal", "end_pos"} & d_members
    if "resume_state" in kw:                                 # the host store carries copies, never the caller's arrays
        for k in ("status", "xstate", "sumacc"):
            assert np.array_equal(out[k], STATE[k]) and out[k] is not STATE[k]
        assert "sample_summary" not in out or (out["sample_summary"] == 1).all()


def shared_arrays(a, b):
    return {k for k, v in a.items() if isinstance(v, np.ndarray) and v is b.get(k)}


def test_host_store_reuses_the_entry_outputs_of_out(library):
    first = _lib.estimate_batch_host(*ARGS, want_state=True, want_smooth=True)
    for v in first.values():
        if isinstance(v, np.ndarray):
            v[...] = 3
    again = _lib.estimate_batch_host(*ARGS, want_state=True, want_smooth=True, out=first)
    assert shared_arrays(again, first) == DRAWS | {"summary", "status"} == set(_lib.ENTRY_OUTPUTS)
    assert (again["status"] == 0).all() and (again["mu"] == 3).all()          # status is zeroed, a draw array stands as it is
    assert all((again[k] == 0).all() for k in ("pi_smooth_mean", "x_final", "pif_final", "xstate", "sumacc"))
    other = _lib.estimate_batch_host(Y, TW, K, 2, 5, (12,), np.zeros((W, 1)), out=first)       # nrun differs: the draws do not fit
    assert shared_arrays(other, first) == {"summary", "status"} and other["mu"].shape == (W, K, 5)
    spoilt = dict(first, summary=first["summary"].astype(np.float32), mu=np.zeros((4, K, W)).T)
    assert shared_arrays(_lib.estimate_batch_host(*ARGS, out=spoilt), spoilt) == DRAWS - {"mu"} | {"status"}


# ---- the derived lists ----
def test_derived_name_lists(library):
    outputs = [r for r in _lib.BUFFERS if r.io == "out"]
    # a skipped window reads NaN in every float output; sumacc, the checkpoint block a RESUME call continues from, is left as it is
    assert set(_lib.NAN_FILLED) == {r.name for r in outputs if r.dtype is np.float64} - {"sumacc"}
    assert set(de.CARRIED) == set(_lib.CARRIED) == {r.name for r in _lib.BUFFERS if r.carried}
    assert set(de.CARRIED) == {"status", "xstate", "sumacc", "sample_summary", "pi_smooth_mean", "pi_filter_mean"}      # include/hmcg.h
    assert de.DRAW_KEYS == _lib.DRAW_KEYS == ("mu", "sig2", "A", "pi_end", "fcast")
    host = _lib.estimate_batch_host(*ARGS)
    collected = de.DeviceCall.collect(types.SimpleNamespace(buf={}, timing=_lib.Timing()))
    untimed = de.DeviceCall.collect(types.SimpleNamespace(buf={}, timing=None))
    assert {k for k, v in host.items() if not isinstance(v, np.ndarray)} == set(collected) - {"_call"} == set(de.TIMING_KEYS)
    assert set(untimed) == set(collected) and all(untimed[k] is None for k in de.TIMING_KEYS)
    assert {"kernel_ms", "steps_per_thread", "occupancy", "buckets", "streaming", "launches", "call_ms"} <= set(de.TIMING_KEYS)


def test_skipped_windows_read_nan_in_the_marked_rows(library):
    state = dict(STATE, status=np.array([0, _lib.ST_NONFINITE, _lib.ST_BAD_T], dtype=np.int32))
    kw = dict(SIGNAL, want_state=True, want_sample_summary=True, want_smooth=True, want_filter_mean=True, want_smooth_draws=True,
              want_corr=True, resume_state=state)
    out = _lib.estimate_batch_host(*ARGS, **kw)
    for k, v in out.items():
        if isinstance(v, np.ndarray) and k != "status":
            assert not np.isnan(v[0]).any() and np.isnan(v[1:]).all() == (k in _lib.NAN_FILLED), k
    assert not any(np.isnan(v).any() for v in _lib.estimate_batch_host(*ARGS, **kw, nan_fill=False).values() if isinstance(v, np.ndarray))


# ---- DevicePanel ----
def test_device_panel_shapes():
    s = device.panel_shapes(3, 7, 2, 4, 1)                   # (W, ldY, K, nrun, H)
    assert {k: s[k] for k in ("mu", "sig2", "A", "pi_end", "fcast", "summary", "status", "corr")} == dict(
        mu=(3, 2, 4), sig2=(3, 2, 4), A=(3, 2, 2, 4), pi_end=(3, 2, 4), fcast=(3, 2, 4), summary=(3, 12), status=(3,), corr=(3, 11, 11))
    s = device.panel_shapes(2, 9, 4, 3, 2)
    assert {k: s[k] for k in ("mu", "sig2", "A", "pi_end", "fcast", "summary", "status", "corr")} == dict(
        mu=(2, 4, 3), sig2=(2, 4, 3), A=(2, 4, 4, 3), pi_end=(2, 4, 3), fcast=(2, 4, 3), summary=(2, 32), status=(2,), corr=(2, 29, 29))
    assert s == _lib.call_shapes(_lib.call_dims(2, 9, 4, 3, 2))
