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
TIMING_KEYS = ("kernel_ms", "threads_per_window", "steps_per_thread", "lds_bytes", "helper_waves", "occupancy", "launches",
               "buckets", "streaming", "call_ms")
DRAW_KEYS = ("mu", "sig2", "A", "pi_end", "fcast")
# what a RESUME call reads back from the caller's buffers
CARRIED = ("status", "xstate", "sumacc", "sample_summary", "pi_smooth_mean", "pi_filter_mean")


class PlaceholderCall:
    """The buffer interface of DeviceCall over made-up non-null addresses: what extras_passed() builds a call on."""

    def __init__(self):
        self.buf, self.inp, self.next = {}, {}, 0x1000

    def upload(self, name, a, dtype):
        self.next += 0x1000
        return self.next

    def alloc(self, name, shape, dtype, prefill):
        self.next += 0x1000
        self.buf[name] = _Placeholder(tuple(shape), self.next)
        return self.buf[name]


class _Placeholder:
    def __init__(self, shape, ptr):
        self.shape, self.ptr = shape, ptr

    def data_ptr(self):
        return self.ptr

    def copy_(self, other):
        pass


class DeviceCall:
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

    def alloc(self, name, shape, dtype, prefill):
        torch = self.torch
        assert dtype in (np.float64, np.int32, np.uint8)
        tdt = {np.float64: torch.float64, np.int32: torch.int32, np.uint8: torch.uint8}[dtype]
        if prefill is None:
            t = torch.zeros(shape, dtype=tdt, device=self.dev)
        elif dtype is np.float64:
            t = torch.full(shape, float("nan"), dtype=tdt, device=self.dev)
        else:
            t = torch.full(shape, SENTINEL_BYTE * (0x01010101 if dtype is np.int32 else 1), dtype=tdt, device=self.dev)
        self.buf[name] = t
        return t

    def collect(self):
        out = {k: t.cpu().numpy() for k, t in self.buf.items()}
        tm = self.timing
        for k in TIMING_KEYS:
            out[k] = None if tm is None else getattr(tm, k)
        if tm is not None:
            out["streaming"] = bool(tm.streaming)
        out["_call"] = self
        return out


def sentinel_like(a):
    """What an untouched output of that dtype holds after the default prefill."""
    if a.dtype == np.float64:
        return np.full(a.shape, np.nan)
    return np.frombuffer(bytes([SENTINEL_BYTE]) * a.nbytes, dtype=a.dtype).reshape(a.shape)


def _build(c, Y, T, K, burnin, nrun, horizons=(12,), yreal=None, seed=1234, window_base=0, window_ids=None,
           threads_per_window=0, alpha=0.0, nu=0.0, x_init=None, want_state=False,
           sig_range=None, save_range=None, sigma_signal=None, kappa=0.0, n_samples=0, end_pos=None, blend_mask=0,
           want_sample_summary=False, want_smooth=False, want_filter_mean=False, want_smooth_draws=False,
           want_corr=False, sweep_base=0, sweep_count=0, resume_state=None,
           min_T=0, max_T=None, prefill=SENTINEL, out=None, pass_pif=True, device=0):
    """Uploads the inputs and allocates the outputs through c (a DeviceCall, or a PlaceholderCall), builds hmcg_config and
    hmcg_extras from the addresses and leaves them in c.launch."""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    W, ldY = Y.shape
    T = np.ascontiguousarray(T, dtype=np.int32)
    H = len(horizons)
    NS = 3 * K + K * K + 2 * H
    ns = max(int(n_samples), 1)
    nd = ns * nrun
    prev = None
    if resume_state is not None and "_call" in resume_state:
        prev = resume_state["_call"]
    elif out is not None:
        prev = out["_call"]
    if prev is not None:
        c.buf = prev.buf                     # the same device buffers: nothing is prefilled, nothing reallocated

    def buf(name, shape, dtype=np.float64):
        t = c.buf.get(name)
        if t is None:
            t = c.alloc(name, shape, dtype, prefill)
            if resume_state is not None and name in CARRIED:
                import torch
                t.copy_(torch.from_numpy(np.ascontiguousarray(resume_state[name], dtype=dtype).reshape(shape)))
        assert tuple(t.shape) == tuple(shape), (name, tuple(t.shape), shape)
        return t.data_ptr()

    dY, dT = c.upload("Y", Y, np.float64), c.upload("T", T, np.int32)
    dyreal = 0 if yreal is None else c.upload("yreal", np.asarray(yreal, dtype=np.float64).reshape(W, H), np.float64)
    shapes = dict(mu=(W, K, nd), sig2=(W, K, nd), A=(W, K, K, nd), pi_end=(W, K, nd), fcast=(W, 2 * H, nd))
    ptr = {name: buf(name, shapes[name]) for name in DRAW_KEYS}
    ptr["summary"] = buf("summary", (W, NS))
    ptr["status"] = buf("status", (W,), np.int32)
    ex = _lib.Extras()
    ex.struct_size = C.sizeof(_lib.Extras)
    flags = 0
    if x_init is not None:
        ex.x_init = c.upload("x_init", np.asarray(x_init).reshape(W, ldY), np.int32)
    if window_ids is not None:
        ex.window_ids = c.upload("window_ids", np.asarray(window_ids).reshape(W), np.uint32)
    if sig_range is not None:
        ex.sig_range = c.upload("sig_range", np.asarray(sig_range).reshape(W, 2), np.int32)
        if save_range is not None:
            svr = np.ascontiguousarray(save_range, dtype=np.int32).reshape(W, 2)
            ex.save_range = c.upload("save_range", svr, np.int32)
            nsave = int(max(1, (svr[:, 1] - svr[:, 0]).max()))
            ex.sigvals = buf("sigvals", (W, ns, nsave))
            ex.nsave_ld = nsave
        if sigma_signal is not None:
            ex.sigma_signal = c.upload("sigma_signal", np.asarray(sigma_signal).reshape(W), np.float64)
        if end_pos is not None:
            ex.end_pos = c.upload("end_pos", np.asarray(end_pos).reshape(W), np.int32)
    if want_sample_summary:
        ex.sample_summary = buf("sample_summary", (W, ns, NS))
    if want_smooth_draws:
        ex.pi_smooth_draws = buf("pi_smooth_draws", (W, K, ldY, nd))
    if want_smooth:
        ex.pi_smooth_mean = buf("pi_smooth_mean", (W, ldY, K))
    if want_filter_mean:
        ex.pi_filter_mean = buf("pi_filter_mean", (W, ldY, K))
    if want_corr:
        NC = 3 * K + K * K + 1
        ex.corr = buf("corr", (W, NC, NC))
    if want_state or ((want_smooth or want_filter_mean or want_smooth_draws) and pass_pif):
        ex.pif_final = buf("pif_final", (W, ldY, K))
    if want_state:
        ex.x_final = buf("x_final", (W, ldY), np.int32)
    if want_state or resume_state is not None:
        ex.xstate = buf("xstate", (W, ldY), np.uint8)
        ex.sumacc = buf("sumacc", (W, NS + K))
    if resume_state is not None:
        flags |= _lib.FLAG_RESUME
    cfg = _lib.make_config(W, K, ldY, min(int(T.max()), ldY) if max_T is None else max_T, burnin, nrun, horizons, seed, window_base,
                           device, flags, threads_per_window, sweep_base, alpha, nu, sweep_count, kappa, n_samples, blend_mask, min_T)
    c.launch = (cfg, (dY, dT, dyreal, ptr["mu"], ptr["sig2"], ptr["A"], ptr["pi_end"], ptr["fcast"], ptr["summary"], ptr["status"]), ex)
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
