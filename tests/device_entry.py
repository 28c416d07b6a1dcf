"""hmcg_estimate_batch_device with the interface of _lib.estimate_batch_host: every buffer a torch tensor in HBM, hmcg_extras
built from device pointers, the result copied back into the same dict of numpy arrays in the same layouts.  A plain module for
the GPU tests (tests/test_gpu_device_entry.py); importing it needs neither torch nor a GPU.

What the device entry leaves to its caller, and the host entry hides, is made visible here:
  * every output is prefilled with a sentinel before the call -- NaN in the float outputs, 0x5a bytes in the integer ones,
    `status` included -- so an element the kernel did not write, or read before writing it, shows in a comparison
    (prefill=None: zeros, what the host entry's own block holds);
  * the buffers a RESUME call reads back (status, xstate, sumacc, sample_summary, pi_smooth_mean, pi_filter_mean) take
    resume_state's contents instead; where resume_state is a result of this runner, its device buffers themselves are the
    call's buffers -- the per-draw arrays included, so a split chain writes into one set of full-length arrays;
  * out=<an earlier result of this runner>: that call's device buffers are used as they stand (dirty), without RESUME.
extras_passed() says which hmcg_extras pointer members a call passes: it builds the call's hmcg_extras with the very code
the runner uses, over placeholder addresses instead of HBM (no torch, no GPU), and reads the struct.  tests/test_variant_coverage.py
holds the case tables of the device-entry tests to include/hmcg.h with it.

prepare_call() uploads, allocates and prefills; DeviceCall.enqueue() is the hmcg_estimate_batch_device call alone, so several
prepared calls can be enqueued back to back with nothing between them."""
import ctypes as C

import numpy as np

from hmc_jl_amd import _lib

SENTINEL = "sentinel"
SENTINEL_BYTE = 0x5A
TIMING_KEYS = tuple(_lib.timing_result(None))
DRAW_KEYS, CARRIED = _lib.DRAW_KEYS, _lib.CARRIED


class _Store:
    """What the two stores of _lib.build_call below share: a buffer of an earlier call is used as it stands; a new one takes
    resume_state's contents where a RESUME call reads it back (CARRIED)."""
    prefill, resume_state = SENTINEL, None

    def alloc(self, name, shape, dtype):
        t = self.buf.get(name)
        if t is None:
            t = self.buf[name] = self.new(shape, dtype)
            if self.resume_state is not None and name in CARRIED:
                self.fill(t, np.ascontiguousarray(self.resume_state[name], dtype=dtype).reshape(shape))
        assert tuple(t.shape) == tuple(shape), (name, tuple(t.shape), shape)
        return t.data_ptr()


class PlaceholderCall(_Store):
    """The buffer interface of DeviceCall over made-up non-null addresses: what extras_passed() builds a call on."""

    def __init__(self):
        self.buf, self.inp, self.next = {}, {}, 0x1000

    def upload(self, name, a, dtype):
        self.next += 0x1000
        return self.next

    def new(self, shape, dtype):
        self.next += 0x1000
        return _Placeholder(tuple(shape), self.next)

    def fill(self, t, a):
        pass


class _Placeholder:
    def __init__(self, shape, ptr):
        self.shape, self.ptr = shape, ptr

    def data_ptr(self):
        return self.ptr


class DeviceCall(_Store):
    """One call's device buffers: filled by prepare_call; enqueue() is the library call; collect() copies everything back."""

    def __init__(self, device=0):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", device)
        self.inp = {}            # inputs, kept alive until the work is done
        self.buf = {}            # outputs and checkpoint blocks, by the host runner's names
        self.timing = None
        self.launch = None       # set by prepare_call: the arguments of hmcg_estimate_batch_device

    def enqueue(self, stream=None, timed=True):
        """hmcg_estimate_batch_device on the prepared buffers, nothing else: no synchronisation before or after (a timed call
        waits inside the library).  stream: a torch.cuda.Stream (None: the library's own)."""
        cfg, ptrs, ex = self.launch
        try:
            self.timing = _lib.estimate_batch_device(cfg, *ptrs, ex, None if stream is None else stream.cuda_stream, timed)
        except _lib.HmcgError as e:
            e.call = self                    # a refused call: its buffers, for the test that nothing was written
            raise
        return self

    def upload(self, name, a, dtype):
        a = np.ascontiguousarray(a, dtype=dtype)
        signed = {np.dtype(np.uint32): np.int32}.get(a.dtype)            # (torch has no arithmetic uint32; the bytes are what travels)
        t = self.torch.from_numpy(a.view(signed) if signed else a).to(self.dev)
        self.inp[name] = t
        return t.data_ptr()

    def new(self, shape, dtype):
        torch = self.torch
        assert dtype in (np.float64, np.int32, np.uint8)
        tdt = {np.float64: torch.float64, np.int32: torch.int32, np.uint8: torch.uint8}[dtype]
        if self.prefill is None:
            return torch.zeros(shape, dtype=tdt, device=self.dev)
        if dtype is np.float64:
            return torch.full(shape, float("nan"), dtype=tdt, device=self.dev)
        return torch.full(shape, SENTINEL_BYTE * (0x01010101 if dtype is np.int32 else 1), dtype=tdt, device=self.dev)

    def fill(self, t, a):
        t.copy_(self.torch.from_numpy(a))

    def collect(self):
        out = {k: t.cpu().numpy() for k, t in self.buf.items()}
        out.update(_lib.timing_result(None if self.timing is None else [self.timing]))
        out["_call"] = self
        return out


def sentinel_like(a):
    """What an untouched output of that dtype holds after the default prefill."""
    if a.dtype == np.float64:
        return np.full(a.shape, np.nan)
    return np.frombuffer(bytes([SENTINEL_BYTE]) * a.nbytes, dtype=a.dtype).reshape(a.shape)


def _build(c, *args, prefill=SENTINEL, out=None, pass_pif=True, resume_state=None, **kw):
    """_lib.build_call over c (a DeviceCall, or a PlaceholderCall) with the device runner's options, left in c.launch."""
    c.prefill, c.resume_state = prefill, resume_state
    prev = resume_state if resume_state is not None and "_call" in resume_state else out
    if prev is not None:
        c.buf = prev["_call"].buf            # the same device buffers: nothing is prefilled, nothing reallocated
    c.launch = _lib.build_call(c, *args, resume=resume_state is not None, pif_with_smoothing=pass_pif, **kw)
    return c


def extras_passed(*args, **kw):
    """The pointer members of hmcg_extras that estimate_batch_device_np(*args, **kw) hands to the library: read from the struct
    the runner's own code builds for that call, over placeholder addresses (no torch, no GPU)."""
    kw = {k: v for k, v in kw.items() if k not in ("stream", "timed", "defer")}
    ex = _build(PlaceholderCall(), *args, **kw).launch[2]
    return {name for name, ty in _lib.Extras._fields_ if ty is C.c_void_p and getattr(ex, name)}


def prepare_call(*args, **kw):
    """Upload, allocate and prefill for one call (the arguments of estimate_batch_device_np but stream / timed / defer); the
    DeviceCall comes back ready for .enqueue().  The fills run on torch's current stream: synchronise before enqueueing."""
    return _build(DeviceCall(kw.get("device", 0)), *args, **kw)


def estimate_batch_device_np(Y, T, K, burnin, nrun, horizons=(12,), yreal=None, stream=None, timed=True, defer=False, **kw):
    """hmcg_estimate_batch_device over torch-allocated HBM buffers; the dict of _lib.estimate_batch_host (numpy arrays in the
    C-ABI layouts, the timing keys -- None when timed=False) plus "_call", the DeviceCall that holds the device buffers.
    Keywords (see _build): those of the host runner -- seed, window_base, window_ids, threads_per_window, alpha, nu, x_init,
    want_state, sig_range, save_range, sigma_signal, kappa, n_samples, end_pos, blend_mask, want_sample_summary, want_smooth,
    want_filter_mean, want_smooth_draws, want_corr, sweep_base, sweep_count, resume_state -- and the device entry's own:
    min_T: hmcg_config.min_T (the length-bucketed dispatch); max_T: hmcg_config.max_T (default min(max T, ldY), as the host runner);
    prefill (SENTINEL, or None for zeros); out (an earlier result whose buffers are reused as they stand);
    pass_pif=False withholds extras.pif_final from a smoothing call that does not ask for the state outputs.
    stream: a torch.cuda.Stream (None: the library's own).  timed=False returns after enqueueing; the runner then waits for
    `stream` alone (or the device, without one) before it copies back -- unless defer=True: the DeviceCall is returned as it is
    and the caller synchronises and calls .collect().
    A refused call raises _lib.HmcgError with the DeviceCall as its .call."""
    import torch
    c = prepare_call(Y, T, K, burnin, nrun, horizons, yreal, **kw)
    torch.cuda.synchronize(c.dev)            # the uploads and fills ran on torch's stream; the library uses its own or the caller's
    c.enqueue(stream, timed)
    if defer:
        return c
    if not timed:
        if stream is not None:
            stream.synchronize()             # the caller's stream alone
        else:
            torch.cuda.synchronize(c.dev)
    return c.collect()


# ---- comparisons between two runs ----
T_AXIS = {"x_final": 0, "xstate": 0, "pif_final": 0, "pi_smooth_mean": 0, "pi_filter_mean": 0, "pi_smooth_draws": 1}   # per window
# (every kernel guards its per-step stores with t < T[w], pif_final included)
UNTOUCHED_BEYOND_T = tuple(T_AXIS)


def arrays_of(g):
    return {k: v for k, v in g.items() if isinstance(v, np.ndarray)}


def assert_device_equals_host(d, h, Tw, save=None):
    """Every array both entries return, bit for bit, over what a window owns: steps t < T[w] of the per-step arrays, the saved
    positions of sigvals.  Beyond it the host entry hands back zeros; the device entry must have left the sentinel."""
    D, Hh = arrays_of(d), arrays_of(h)
    assert set(D) <= set(Hh), sorted(set(D) - set(Hh))
    for k, dv in D.items():
        hv = Hh[k]
        assert dv.shape == hv.shape and dv.dtype == hv.dtype, (k, dv.shape, hv.shape, dv.dtype, hv.dtype)
        for w, T in enumerate(Tw):
            x, y = dv[w], hv[w]
            if k in T_AXIS:
                ax = T_AXIS[k]
                rest = np.take(x, range(int(T), x.shape[ax]), axis=ax)
                x, y = np.take(x, range(int(T)), axis=ax), np.take(y, range(int(T)), axis=ax)
                if k in UNTOUCHED_BEYOND_T:
                    assert np.array_equal(rest, sentinel_like(rest), equal_nan=True), (k, w, "written beyond T")
            elif k == "sigvals" and save is not None:
                n = int(save[w][1] - save[w][0])
                x, y = x[:, :n], y[:, :n]
            assert np.array_equal(x, y, equal_nan=True), (k, w)


def kept_after(sweeps, burnin, nrun, n_samples):
    """Kept draws of the first `sweeps` sweeps (sample-major on the signal path)."""
    per = burnin + nrun
    full, rem = divmod(sweeps, per)
    return min(full, n_samples) * nrun + (max(0, rem - burnin) if full < n_samples else 0)
