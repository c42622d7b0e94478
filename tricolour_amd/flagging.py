"""Host-side mirror of ``tricolour.flagging.sum_threshold_flagger``.

Same name, keyword arguments, defaults, return value and error behaviour as
the reference (``tricolour/flagging.py:1076-1196``); the numerics run in the
HIP extension through the C ABI (``include/tricolour_amd.h``).  PyTorch is
only used to own device memory and the HIP stream.

* ``numpy`` in -> ``numpy`` out (H2D, run, D2H);
* ``torch`` ROCm tensors in -> ``torch.bool`` tensor out on the same device,
  zero-copy, enqueued on the current stream.

There is no CPU path: without a GPU (or without the built extension) the
call raises ``RuntimeError``.
"""
import ctypes as C
import collections
import functools
import os
import threading
import time

import numpy as np

from tricolour_amd import _lib

_tls = threading.local()
# host-array calls take turns on the PCIe link (TRICOLOUR_AMD_LINK_TURNS=0: free-for-all)
_H2D_TURN = threading.Lock()
_D2H_TURN = _H2D_TURN
_LINK_TURNS = os.environ.get("TRICOLOUR_AMD_LINK_TURNS", "1") != "0"
_TRACE = [] if os.environ.get("TRICOLOUR_AMD_TRACE") == "1" else None   # (debug) per-call phase times
# numpy blocks are cut into up to this many pieces along the baseline axis and pipelined inside the call
# (copy of piece i + 1 under the kernels of piece i); TRICOLOUR_AMD_PIPELINE=1 keeps a block in one piece
# (2 pieces measured best for one calling thread: 128 -> 102 ms per 16-baseline block; 4 pieces: 110 ms, the launches get
# too small.  When other threads have calls in flight their blocks already overlap each other's copies: no cutting then.)
_PIPELINE_PIECES = int(os.environ.get("TRICOLOUR_AMD_PIPELINE", "2") or 1)
_PIPELINE_MIN_WINDOWS = 16         # (bl, corr) windows per piece at least: smaller launches no longer fill the device
_INFLIGHT = [0]                    # numpy-block calls currently inside the library (all threads)
_INFLIGHT_LOCK = threading.Lock()
_LAST_CALLER = [None, 0.0]         # (thread id, time) of the latest numpy-block call
# TRICOLOUR_AMD_PINNED_RESULTS=1: numpy results are views of pinned host tensors from torch's caching host allocator --
# the flags then land in the result array at the link rate, without the 20 ms CPU copy into freshly mapped pages per
# 16-baseline block.  Opt-in: every result the caller keeps alive pins its memory.
_PINNED_RESULTS = os.environ.get("TRICOLOUR_AMD_PINNED_RESULTS", "0") == "1"


def _torch():
    import torch
    return torch


def _require_gpu():
    torch = _torch()
    _lib.lib()  # fail loudly if the extension is missing
    if not torch.cuda.is_available():
        raise RuntimeError("tricolour_amd needs a ROCm GPU (MI355X / gfx950); "
                           "no device is visible and there is no CPU fallback")
    return torch


def prepare_params(ntime, nchan, outlier_nsigma=4.5,
                   windows_time=[1, 2, 4, 8], windows_freq=[1, 2, 4, 8],
                   background_reject=2.0, background_iterations=1,
                   spike_width_time=12.5, spike_width_freq=10.0,
                   time_extend=3, freq_extend=3,
                   freq_chunks=10, average_freq=1,
                   flag_all_time_frac=0.6, flag_all_freq_frac=0.8,
                   rho=1.3, num_major_iterations=5):
    """The plain-Python preparation of ``flagging.py:1156-1179`` (window
    de-duplication and clipping, frequency chunk ends), done by the library's
    ``tri_prepare_params``.  Returns a ``TriParams`` (keeps its chunk buffer
    alive) -- usable without a GPU."""
    lib = _lib.lib()
    wt = (C.c_double * max(len(windows_time), 1))(*[float(w) for w in windows_time])
    wf = (C.c_double * max(len(windows_freq), 1))(*[float(w) for w in windows_freq])
    freq_chunks = int(freq_chunks)
    buf = (C.c_int64 * (max(freq_chunks, 0) + 1))()
    p = _lib.TriParams()
    _lib.check(lib.tri_prepare_params(
        int(ntime), int(nchan), float(outlier_nsigma),
        wt, len(windows_time), wf, len(windows_freq),
        float(background_reject), int(background_iterations),
        float(spike_width_time), float(spike_width_freq),
        int(time_extend), int(freq_extend), freq_chunks, int(average_freq),
        float(flag_all_time_frac), float(flag_all_freq_frac), float(rho),
        int(num_major_iterations), buf, len(buf), C.byref(p)))
    p._chunk_buf = buf
    return p


_WS_CACHE_MAX = 3       # cached workspaces per thread and device (least recently used goes first)


def _workspace(torch, device, nbytes):
    """Per-thread, per-device, per-STREAM workspace tensor (grown on demand): calls from the
    threads of a dask ThreadPool never share scratch memory, and neither do two pipelines
    that one thread has in flight on different streams.  The cache is a small LRU: a thread
    that rotates through many streams keeps at most _WS_CACHE_MAX workspaces per device alive
    (a stream handle can also be recycled by the runtime after its stream is destroyed, so an
    old entry must not live forever); before a workspace GROWS, the thread's other workspaces
    on that device are dropped -- the new one was sized against the memory they hold.  Callers
    that create and destroy streams freely should call release_workspace() when done."""
    cache = getattr(_tls, "ws", None)
    if cache is None:
        cache = _tls.ws = collections.OrderedDict()
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
    t = cache.get(key)
    if t is not None and t.numel() >= nbytes:
        cache.move_to_end(key)
        return t
    if t is not None:
        # this stream's workspace must GROW: it was sized against the memory the thread's other workspaces on the
        # device hold, so those go first (a miss for a new stream leaves them alone -- two pipelined pieces on two
        # side streams keep one workspace each)
        for k in [k for k in cache if k[:2] == key[:2]]:
            del cache[k]
        t = None
    t = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    cache[key] = t
    cache.move_to_end(key)
    mine = [k for k in cache if k[:2] == key[:2]]
    for k in mine[:-_WS_CACHE_MAX]:
        del cache[k]
    return t


def release_workspace():
    """Drops this thread's cached device workspaces."""
    _tls.ws = collections.OrderedDict()


def set_num_threads(n):
    """Declares how many host threads will call into the library concurrently (dask's
    ThreadPool size): every thread then sizes its workspace against 1/n of the device
    instead of against whatever the other threads have left free.  Also settable through
    the environment variable TRICOLOUR_AMD_THREADS."""
    global _declared_threads
    _declared_threads = max(1, int(n))


_declared_threads = None


def _workspace_budget(torch, device, share=1.0):
    """Bytes a call may take for its workspace.  `share`: fraction of the device's free memory this call may claim
    (the in-call pipeline runs two pieces on two streams: each budgets half)."""
    env = os.environ.get("TRICOLOUR_AMD_WORKSPACE_GB")
    if env:
        return int(float(env) * (1 << 30) * share)
    free, total = torch.cuda.mem_get_info(device)
    # what this thread already holds FOR THIS STREAM can be reused or released: it counts as available.  The workspaces
    # of its other streams do not -- they may be in flight, and their blocks return to another stream's pool
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
    mine = getattr(_tls, "ws", {}).get(key)
    have = mine.numel() if mine is not None else 0
    nthreads = _declared_threads or int(os.environ.get("TRICOLOUR_AMD_THREADS", "0") or 0)
    if nthreads > 1:
        # a fixed share of the device -- but never more than what is actually free right now (the caller's own
        # slabs, other processes): the batch shrinks instead of the allocation failing
        return max(min(int(0.6 * total / nthreads * share), int(0.9 * free * share) + have), 0)
    return int(0.6 * (free * share + have))


def _pick_batch(lib, p, n_cp, T, F, budget):
    one = lib.tri_workspace_bytes(1, T, F, C.byref(p))
    if one == 0:
        # let the flagger produce the precise error message
        return 1, 256
    if one > budget:
        raise MemoryError("tricolour_amd: one (%d x %d) window needs %.1f MiB of "
                          "workspace, more than the %.1f MiB budget"
                          % (T, F, one / 2**20, budget / 2**20))
    lo, hi = 1, max(1, min(n_cp, 4096))
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if lib.tri_workspace_bytes(mid, T, F, C.byref(p)) <= budget:
            lo = mid
        else:
            hi = mid - 1
    return lo, lib.tri_workspace_bytes(lo, T, F, C.byref(p))


def _window_batch(n_win, ws_bytes, budget, launch_cap=None, max_windows=None):
    """``(batch, nbytes)``: windows per library call of a strategy step and the workspace they need.  All ``n_win``,
    capped by what one launch holds (``launch_cap``, each family's own figure) and by ``max_windows`` (how tests force
    batches), then halved until ``ws_bytes(batch)`` fits ``budget``: an int, or a callable asked only if a workspace is
    needed at all.  At least one window.  Pure arithmetic."""
    batch = n_win if launch_cap is None else max(1, min(n_win, launch_cap))
    if max_windows:
        batch = max(1, min(batch, int(max_windows)))
    nbytes = ws_bytes(batch)
    if nbytes > 0:
        if callable(budget):
            budget = budget()
        while batch > 1 and ws_bytes(batch) > budget:
            batch = (batch + 1) // 2
        nbytes = ws_bytes(batch)
    return batch, nbytes


def _batches(n_win, batch):
    """``(w0, b)``: the first window and the number of windows of every batch."""
    for w0 in range(0, n_win, batch):
        yield w0, min(batch, n_win - w0)


def _at(t, n_win, w0):
    """Address of window ``w0`` of a contiguous tensor that holds ``n_win`` windows (None stays None)."""
    return None if t is None else t.data_ptr() + w0 * (t.numel() // n_win) * t.element_size()


def _window_launches(torch, device, n_win, ws_bytes, launch_cap=None, max_windows=None, workspace=True):
    """The frame of a batched step on the current device: its batches, sized against this call's budget, as ``(at, b)``
    -- ``at(t)``: :func:`_at` of the batch's first window, ``b``: its windows -- and the ``(workspace, its bytes, stream)``
    that end a batched entry point's arguments: this thread's workspace, or ``None, 0`` if none is needed or taken."""
    batch, nbytes = _window_batch(n_win, ws_bytes, lambda: _workspace_budget(torch, device), launch_cap, max_windows)
    ws = _workspace(torch, device, nbytes) if nbytes > 0 and workspace else None
    stream = torch.cuda.current_stream(device).cuda_stream
    launches = ((functools.partial(_at, n_win=n_win, w0=w0), b) for w0, b in _batches(n_win, batch))
    return launches, ((ws.data_ptr(), ws.numel(), stream) if ws is not None else (None, 0, stream))


def _host_call_stream(torch, vis, flags):
    """Calls that hand over HOST arrays (the dask graph does) run on a stream of
    their own, one per calling thread: the H2D copies, kernels and the D2H copy
    of blocks processed by different threads then overlap instead of queueing
    on the default stream.  Device tensors stay on the caller's current stream."""
    for a in (vis, flags):
        if torch.is_tensor(a) and a.is_cuda:
            return None
    device = torch.device("cuda", torch.cuda.current_device())
    streams = getattr(_tls, "streams", None)
    if streams is None:
        streams = _tls.streams = {}
    key = device.index
    if key not in streams:
        streams[key] = torch.cuda.Stream(device)
    return streams[key]


_D2H_STAGE_MAX = 1 << 30      # larger results (blocks of > 64 baselines of 1024 x 4096) go straight to their array


def _d2h_stage(torch, nbytes):
    """This thread's pinned staging buffer for results (grown on demand, reused by every later call);
    None when the result is too large to keep pinned memory of its size around, or pinning fails."""
    if nbytes > _D2H_STAGE_MAX:
        return None
    st = getattr(_tls, "d2h_stage", None)
    if st is None or st.numel() < nbytes:
        _tls.d2h_stage = None
        try:
            st = _tls.d2h_stage = torch.empty(int(nbytes), dtype=torch.uint8).pin_memory()
        except RuntimeError:
            return None
    return st


def _as_device_inputs(torch, vis, flags):
    """Returns (vis_tensor, flags_u8_tensor, vis_dtype_code, from_numpy, device)."""
    from_numpy = isinstance(vis, np.ndarray) or isinstance(flags, np.ndarray)
    device = None
    if torch.is_tensor(vis) and vis.is_cuda:
        device = vis.device
    elif torch.is_tensor(flags) and flags.is_cuda:
        device = flags.device
    else:
        device = torch.device("cuda", torch.cuda.current_device())

    def to_t(a):
        if isinstance(a, np.ndarray):
            # pageable host memory: the driver's own staged copy runs at the link rate on this platform
            # (56 GB/s measured, scripts/host_copy_rates.py) -- faster than copying into pinned buffers first
            return torch.from_numpy(np.ascontiguousarray(a)).to(device, non_blocking=True)
        if torch.is_tensor(a):
            return a.to(device)
        return torch.as_tensor(np.asarray(a)).to(device)

    if from_numpy and _LINK_TURNS:
        # One block on the link at a time.  A single copy already saturates it, so queueing the copies
        # loses nothing -- but it staggers the calling threads: while one block's kernels run, the next
        # thread's block is on the link, instead of all threads copying together and then computing
        # together (measured: 2.2 -> see profiles/r02_host_path.txt).
        t0 = time.time()
        with _H2D_TURN:
            t1 = time.time()
            v = to_t(vis)
            f = to_t(flags)
            torch.cuda.current_stream(device).synchronize()
        if _TRACE is not None:
            _TRACE.append((threading.get_ident(), "h2d", t0, t1, time.time()))
    else:
        v = to_t(vis)
        f = to_t(flags)
    if v.dtype == torch.complex64:
        code = _lib.TRI_VIS_C64
    elif v.dtype == torch.float32:
        code = _lib.TRI_VIS_F32
    elif v.dtype == torch.float64:
        # |x| of a float64 enters the reference's float32 accumulator through
        # one round-to-nearest (flagging.py:856-859), which is what the cast
        # does when no channel averaging follows
        code = -64
    elif v.dtype == torch.complex128:
        code = -128
    else:
        raise TypeError("tricolour_amd.sum_threshold_flagger: visibilities must be real or "
                        "complex floating point (got %s)" % v.dtype)
    if f.dtype == torch.bool:
        f8 = f.contiguous().view(torch.uint8)
    elif f.dtype in (torch.uint8, torch.int8):
        f8 = f.contiguous().view(torch.uint8)
    else:
        f8 = (f != 0).view(torch.uint8)   # flagging.py:833-835: non-zero = flagged
    return v.contiguous(), f8, code, from_numpy, device


def sum_threshold_flagger(vis, flags, outlier_nsigma=4.5,
                          windows_time=[1, 2, 4, 8], windows_freq=[1, 2, 4, 8],
                          background_reject=2.0, background_iterations=1,
                          spike_width_time=12.5, spike_width_freq=10.0,
                          time_extend=3, freq_extend=3,
                          freq_chunks=10, average_freq=1,
                          flag_all_time_frac=0.6, flag_all_freq_frac=0.8,
                          rho=1.3, num_major_iterations=5, _debug=None):
    """
    Flagger that uses the SumThreshold method (Offringa, A., MNRAS, 405,
    155-167, 2010) to detect spikes in both frequency and time axes --
    MI355X implementation of ``tricolour.flagging.sum_threshold_flagger``
    (reference ``tricolour/flagging.py:1076-1196``), same arguments:

    vis : (bl, corr, time, chan) complex64 (or float32 amplitudes)
    flags : same shape, bool (any integer type: non-zero = flagged)

    Returns the flags found by the LAST major iteration (not OR-ed with the
    input flags), bool, same 4-D shape; inputs are never modified.
    """
    lib = _lib.lib()
    if tuple(vis.shape) != tuple(flags.shape):
        raise ValueError("shape mismatch")           # flagging.py:840-841
    if len(vis.shape) != 4:
        raise ValueError("not enough values to unpack (expected 4, got %d)"
                         % len(vis.shape))            # flagging.py:1156
    nbl, ncorr, ntime, nchan = (int(s) for s in vis.shape)
    p = prepare_params(ntime, nchan, outlier_nsigma, windows_time, windows_freq,
                       background_reject, background_iterations, spike_width_time,
                       spike_width_freq, time_extend, freq_extend, freq_chunks,
                       average_freq, flag_all_time_frac, flag_all_freq_frac, rho,
                       num_major_iterations)
    torch = _require_gpu()
    if _debug is None and isinstance(vis, np.ndarray) and isinstance(flags, np.ndarray):
        me, now = threading.get_ident(), time.time()
        with _INFLIGHT_LOCK:
            _INFLIGHT[0] += 1
            # alone: nobody else inside, and no other thread was here within the last two seconds (a pool of
            # threads taking blocks one after the other overlaps their copies by itself)
            alone = _INFLIGHT[0] == 1 and (_LAST_CALLER[0] in (None, me) or now - _LAST_CALLER[1] > 2.0)
            _LAST_CALLER[0], _LAST_CALLER[1] = me, now
        try:
            if (alone and _PIPELINE_PIECES > 1 and nbl >= 2 and nbl * ncorr >= 2 * _PIPELINE_MIN_WINDOWS
                    and ntime > 0 and nchan > 0):
                return _flag_numpy_pipelined(torch, lib, p, vis, flags, average_freq)
            return _flag_host_call(torch, lib, p, vis, flags, average_freq, _debug)
        finally:
            with _INFLIGHT_LOCK:
                _INFLIGHT[0] -= 1
                _LAST_CALLER[1] = time.time()
    return _flag_host_call(torch, lib, p, vis, flags, average_freq, _debug)


def _flag_host_call(torch, lib, p, vis, flags, average_freq, _debug):
    side = _host_call_stream(torch, vis, flags)
    if side is not None:
        caller = torch.cuda.current_stream(side.device)
        side.wait_stream(caller)          # anything the caller queued (e.g. a CPU tensor being produced) comes first
        with torch.cuda.stream(side):
            out = _flag_on_current_stream(torch, lib, p, vis, flags, average_freq, _debug)
        if torch.is_tensor(out) and out.is_cuda:
            # host inputs that were not numpy (CPU tensors, lists) get a device tensor back: hand it
            # over to the caller's stream properly
            caller.wait_stream(side)
            out.record_stream(caller)
        return out
    return _flag_on_current_stream(torch, lib, p, vis, flags, average_freq, _debug)


def _flag_numpy_pipelined(torch, lib, p, vis, flags, average_freq):
    """One numpy block, pipelined INSIDE the call (the dask graph hands over one block per call and thread,
    dask_wrappers.py:23-46 of the reference): the block is cut into pieces along the baseline axis, piece i + 1 is
    on the PCIe link while piece i's kernels run (two per-thread side streams, each with its own workspace),
    and piece i's flags come back -- and are copied into the result array by the CPU -- under piece i + 1's
    kernels.  Windows are independent (flagging.py:765-774), so the pieces' results are the block's results."""
    nbl, ncorr, ntime, nchan = (int(x) for x in vis.shape)
    device = torch.device("cuda", torch.cuda.current_device())
    pieces = max(2, min(_PIPELINE_PIECES, nbl, (nbl * ncorr) // _PIPELINE_MIN_WINDOWS))
    bounds = [nbl * k // pieces for k in range(pieces + 1)]
    streams = getattr(_tls, "pipe_streams", None)
    if streams is None:
        streams = _tls.pipe_streams = {}
    if device.index not in streams:
        streams[device.index] = (torch.cuda.Stream(device), torch.cuda.Stream(device))
    pair = streams[device.index]
    caller = torch.cuda.current_stream(device)
    res = _new_result(torch, (nbl, ncorr, ntime, nchan))
    pending = None

    def drain(item):
        out, st, b0, b1 = item
        with torch.cuda.stream(st):
            _result_to_numpy(torch, out, device, res[b0:b1])
    for k in range(pieces):
        b0, b1 = bounds[k], bounds[k + 1]
        if b1 <= b0:
            continue
        st = pair[k & 1]
        st.wait_stream(caller)
        with torch.cuda.stream(st):
            out, _ = _flag_device(torch, lib, p, vis[b0:b1], flags[b0:b1], average_freq, None, share=0.5)
        if pending is not None:
            drain(pending)          # (its kernels were queued before this piece's copy: they ran under it)
        pending = (out, st, b0, b1)
    if pending is not None:
        drain(pending)
    return res


def _flag_on_current_stream(torch, lib, p, vis, flags, average_freq, _debug):
    out, from_numpy = _flag_device(torch, lib, p, vis, flags, average_freq, _debug)
    if from_numpy:
        return _result_to_numpy(torch, out, out.device)
    return out


def _flag_device(torch, lib, p, vis, flags, average_freq, _debug, share=1.0):
    """Inputs to the device (if they are not there), the flagger on the current stream; returns the device
    bool tensor and whether the caller handed over numpy arrays."""
    nbl, ncorr, ntime, nchan = (int(s) for s in vis.shape)
    v, f8, code, from_numpy, device = _as_device_inputs(torch, vis, flags)
    nan_part = None
    if code in (-64, -128):
        # float64 / complex128 input (the reference accepts "real or complex", flagging.py:830-835):
        # its amplitude is np.abs in float64 -- for complex128 numba's hypot(re, im) -- and enters the
        # float32 accumulator `value` through one round-to-nearest (flagging.py:856-859).  Without
        # channel averaging that rounded amplitude IS the averaged sample, so it can be formed up front.
        # With channel averaging the float64 amplitude itself enters the accumulator -- the sum is formed in float64 and
        # rounded to float32 at every step (flagging.py:858-859) -- so it goes to the library as float64 (TRI_VIS_F64); a
        # visibility with a NaN part arrives as NaN (the final isnan(in_data), flagging.py:777-781).
        wide = int(average_freq) != 1
        if code == -128:
            re, im = v.real, v.imag
            # torch.hypot is within 1 ulp of float64 of libm's hypot: far inside the float32 rounding that follows;
            # (inf, nan) -> inf like C99 hypot
            amp = torch.hypot(re, im)
            amp = torch.where(torch.isinf(re) | torch.isinf(im), torch.full_like(amp, float("inf")), amp)
            # A NaN part always flags the sample in the end (flagging.py:777-781), also next to an infinite one -- but the
            # AMPLITUDE of (inf, nan) is +inf (np.abs = hypot), and that is what _average_freq accumulates while the sample
            # is unflagged (flagging.py:856-861).  So the amplitude stays +inf (as on the complex64 route: k_amplitude4
            # keeps amplitude and NaN bit apart) and the NaN marks are OR-ed into the result below.
            nan_part = torch.isnan(re) | torch.isnan(im)
            if not bool((nan_part & torch.isinf(amp)).any()):
                nan_part = None                       # every NaN part already shows as a NaN amplitude
        else:
            amp = v.abs()
        if wide:
            v, code = amp.contiguous(), _lib.TRI_VIS_F64
        else:
            v, code = amp.to(torch.float32), _lib.TRI_VIS_F32
    n_cp = nbl * ncorr
    with torch.cuda.device(device):
        out = torch.empty((nbl, ncorr, ntime, nchan), dtype=torch.uint8, device=device)
        if n_cp > 0 and ntime > 0 and nchan > 0:
            budget = _workspace_budget(torch, device, share)
            _batch, nbytes = _pick_batch(lib, p, n_cp, ntime, nchan, budget)
            ws = _workspace(torch, device, nbytes)
            stream = torch.cuda.current_stream(device).cuda_stream
            if _debug is None:
                rc = lib.tri_sum_threshold_flagger(v.data_ptr(), code, f8.data_ptr(),
                                                   out.data_ptr(), n_cp, ntime, nchan,
                                                   C.byref(p), ws.data_ptr(), ws.numel(),
                                                   stream)
            else:
                fa = (nchan + int(average_freq) - 1) // int(average_freq)
                n = ntime * fa
                dbg_f = torch.zeros(fa + 2 * n, dtype=torch.float32, device=device)
                dbg_u = torch.zeros(fa + 2 * n, dtype=torch.uint8, device=device)
                rc = lib.tri_sum_threshold_flagger_debug(
                    v.data_ptr(), code, f8.data_ptr(), out.data_ptr(), n_cp, ntime,
                    nchan, C.byref(p), ws.data_ptr(), ws.numel(), stream,
                    dbg_f.data_ptr(), dbg_u.data_ptr())
                if rc == 0:
                    torch.cuda.synchronize(device)
                    df, du = dbg_f.cpu().numpy(), dbg_u.cpu().numpy()
                    _debug.update(
                        spec_resid=df[:fa].copy(),
                        background=df[fa:fa + n].reshape(fa, ntime).T.copy(),
                        residual=df[fa + n:].reshape(ntime, fa).copy(),
                        spec_flags=du[:fa].astype(bool),
                        time_flags=du[fa:fa + n].reshape(ntime, fa).astype(bool),
                        freq_flags=du[fa + n:].reshape(ntime, fa).astype(bool))
            _lib.check(rc)
            if nan_part is not None and int(p.num_major_iterations) > 0:
                out |= nan_part.view(torch.uint8)     # flagging.py:777-781 for (inf, nan) samples of complex128 input
        elif ntime <= 0 or nchan <= 0:
            _lib.check(lib.tri_sum_threshold_flagger(
                v.data_ptr(), code, f8.data_ptr(), out.data_ptr(), n_cp, ntime, nchan,
                C.byref(p), None, 0, None))
    return out.view(torch.bool), from_numpy


def _new_result(torch, shape):
    """The numpy bool array a host call returns: ordinary memory, or (TRICOLOUR_AMD_PINNED_RESULTS=1) a view of a pinned
    tensor from torch's caching host allocator (the array keeps the tensor alive; its memory returns to the pool with it)."""
    if _PINNED_RESULTS:
        try:
            return torch.empty(shape, dtype=torch.bool, pin_memory=True).numpy()
        except RuntimeError:
            pass
    return np.empty(shape, np.bool_)


def _dest_is_pinned(torch, dest):
    try:
        return _PINNED_RESULTS and dest is not None and torch.from_numpy(dest).is_pinned()
    except Exception:
        return False


def _result_to_numpy(torch, out, device, dest=None):
    """Device flags of a numpy call -> a fresh numpy bool array, or the C-contiguous array `dest` (on the current stream)."""
    shape = tuple(int(x) for x in out.shape)
    if _PINNED_RESULTS:
        if dest is None:
            dest = _new_result(torch, shape)
        if _dest_is_pinned(torch, dest):
            torch.cuda.current_stream(device).synchronize()
            with _D2H_TURN:
                torch.from_numpy(dest).copy_(out, non_blocking=True)
                torch.cuda.current_stream(device).synchronize()
            return dest
    if _LINK_TURNS:
        t0 = time.time()
        torch.cuda.current_stream(device).synchronize()     # kernels done before queueing for the link
        t1 = time.time()
        # The result goes to a fresh numpy array, whose pages the kernel has to zero and map first:
        # copied into directly, that happens page by page INSIDE the device-to-host copy (5-10 GB/s, and
        # it drags down a concurrent host-to-device copy of another thread).  So: device -> this thread's
        # pinned staging buffer at the link rate (5 ms for a 16-baseline block), link released, then a
        # plain CPU copy into the fresh array.
        stage = _d2h_stage(torch, out.numel())
        if stage is None:
            with _D2H_TURN:
                got = out.cpu().numpy()
            if dest is None:
                return got
            np.copyto(dest, got)
            return dest
        with _D2H_TURN:
            t2 = time.time()
            stage[:out.numel()].copy_(out.view(torch.uint8).reshape(-1), non_blocking=True)
            torch.cuda.current_stream(device).synchronize()
        t3 = time.time()
        res = np.empty(shape, np.bool_) if dest is None else dest
        np.copyto(res.reshape(-1).view(np.uint8), stage[:out.numel()].numpy())
        if _TRACE is not None:
            _TRACE.append((threading.get_ident(), "kernels+d2h", t0, t1, t2, t3, time.time()))
        return res
    got = out.cpu().numpy()
    if dest is None:
        return got
    np.copyto(dest, got)
    return dest


# ---------------------------------------------------------------------------
# The cheap strategy steps around sum_threshold, same
# signatures as the reference so a default.yaml chain can stay on the device.
# ---------------------------------------------------------------------------
def _flags_u8(torch, f, device):
    if isinstance(f, np.ndarray):
        f = torch.from_numpy(np.ascontiguousarray(f))
    f = f.to(device)
    if f.dtype in (torch.bool, torch.uint8, torch.int8):
        return f.contiguous().view(torch.uint8)
    return (f != 0).view(torch.uint8)


def flag_nans_and_zeros(vis_windows, flag_windows):
    """Flag nan and zero visibilities -- ``tricolour.flagging.flag_nans_and_zeros``
    (flagging.py:29-62): ``(vis == 0) | isnan(vis) | (flags != 0)``; output has
    the dtype of ``flag_windows`` (np.zeros_like, flagging.py:51)."""
    if tuple(vis_windows.shape) != tuple(flag_windows.shape):
        raise ValueError("vis_windows.shape != flag_windows.shape")   # flagging.py:46-47
    torch = _require_gpu()
    v, f8, code, from_numpy, device = _as_device_inputs(torch, vis_windows, flag_windows)
    if code == -64:
        raise TypeError("tricolour_amd.flag_nans_and_zeros: visibilities must be complex64 or float32")
    f8 = _flags_u8(torch, flag_windows, device)
    out = torch.empty(f8.shape, dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().tri_flag_nans_and_zeros(
            v.data_ptr(), code, f8.data_ptr(), out.data_ptr(), out.numel(),
            torch.cuda.current_stream(device).cuda_stream))
    return _like_flags(torch, out, flag_windows, from_numpy)


def _like_flags(torch, out_u8, like, from_numpy):
    """uint8 0/1 result -> the container / dtype of the reference's output."""
    if from_numpy:
        o = out_u8.cpu().numpy()
        dt = like.dtype if isinstance(like, np.ndarray) else np.bool_
        return o.view(np.bool_) if dt == np.bool_ else o.astype(dt)
    if torch.is_tensor(like) and like.dtype != torch.bool:
        return out_u8.to(like.dtype)
    return out_u8.view(torch.bool)


def _like_input(from_numpy, *tensors):
    """Device results -> what the caller gets: numpy arrays for numpy input, the tensors otherwise (a tuple)."""
    return tuple(t.cpu().numpy() for t in tensors) if from_numpy else tensors


def _apply_bl_chan(torch, flags, bl_sel, chan_masks, mode):
    from_numpy = isinstance(flags, np.ndarray)
    device = flags.device if (torch.is_tensor(flags) and flags.is_cuda) else \
        torch.device("cuda", torch.cuda.current_device())
    f8 = _flags_u8(torch, flags, device)
    nbl, ncorr, ntime, nchan = (int(x) for x in f8.shape)
    out = f8.clone()                                   # flagging.py:90, 151: flags.copy()
    sel = torch.from_numpy(np.ascontiguousarray(bl_sel, np.uint8)).to(device)
    lib = _lib.lib()
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        for cm in chan_masks:
            m = torch.from_numpy(np.ascontiguousarray(cm, np.uint8)).to(device)
            _lib.check(lib.tri_apply_baseline_channel_mask(
                out.data_ptr(), out.data_ptr(), sel.data_ptr(), m.data_ptr(), mode,
                nbl, ncorr, ntime, nchan, stream))
    return _like_flags(torch, out, flags, from_numpy)


def flag_autos(flags, ubl):
    """Flags auto-correlations -- ``tricolour.flagging.flag_autos``
    (flagging.py:65-95).  ``ubl`` arrives wrapped in a list, as dask's
    ``bl-comp`` contraction delivers it (flagging.py:84)."""
    ubl = np.asarray(ubl[0])
    if flags.shape[0] != ubl.shape[0]:
        raise ValueError("flag and ubl shape mismatch %s != %s" % (flags.shape[2], ubl.shape[0]))
    torch = _require_gpu()
    bl_sel = ubl[:, 1] == ubl[:, 2]
    return _apply_bl_chan(torch, flags, bl_sel, [np.ones(int(flags.shape[3]), np.uint8)], 0)


def static_mask_selection(ubl, antspos, masks, chan_freqs, chan_widths, uvrange=""):
    """Host half of ``apply_static_mask`` (flagging.py:131-160): the baseline
    selection from the uv-range and one boolean channel mask per static mask."""
    from tricolour_amd.util import casa_style_range
    uvrange = casa_style_range(uvrange)
    ubl = np.asarray(ubl)
    antspos = np.asarray(antspos)
    spw_chanlb = chan_freqs - chan_widths * 0.5
    spw_chanub = chan_freqs + chan_widths * 0.5
    bl_length = antspos[ubl[:, 1]] - antspos[ubl[:, 2]]
    d2 = 0.5 * np.sum(bl_length**2, axis=1)
    luvrange = 0.0 if uvrange is None else min(uvrange[0], uvrange[1])
    uuvrange = np.inf if uvrange is None else max(uvrange[0], uvrange[1])
    bl_sel = np.logical_and(d2 >= luvrange**2, d2 <= uuvrange**2)
    chan_masks = []
    for mask in masks:
        mask = np.asarray(mask)
        if mask.ndim != 2 and mask.shape[1] != 1:
            raise ValueError("masks.shape != (dim, 1)")
        lower_mask = mask[:, :] >= spw_chanlb[None, :]
        upper_mask = mask[:, :] < spw_chanub[None, :]
        chan_masks.append(np.logical_and(lower_mask, upper_mask).sum(axis=0) > 0)
    return bl_sel, chan_masks


def apply_static_mask(flag, ubl, antspos, masks, chan_freqs, chan_widths,
                      accumulation_mode="or", uvrange=""):
    """Applies static masks -- ``tricolour.flagging.apply_static_mask``
    (flagging.py:98-172): channels whose band contains a masked frequency are
    flagged ("or") or replace the flags ("override") on the baselines inside
    ``uvrange``."""
    ubl = np.asarray(ubl)
    if flag.shape[0] != ubl.shape[0]:
        raise ValueError("flag and ubl shape mismatch %s != %s" % (flag.shape[1], ubl.shape[0]))
    if accumulation_mode not in ("or", "override"):
        if len(masks) > 0:
            raise ValueError("Invalid accumulation_mode '%s'. Should be 'or' or 'override'"
                             % accumulation_mode)
    bl_sel, chan_masks = static_mask_selection(ubl, antspos, masks, chan_freqs, chan_widths, uvrange)
    torch = _require_gpu()
    return _apply_bl_chan(torch, flag, bl_sel, chan_masks, 0 if accumulation_mode == "or" else 1)


def uvcontsub_flagger(vis, flags, major_cycles=5, or_original_from_cycle=1,
                      taylor_degrees=20, sigma=5):
    """Iteratively fits a low-order Fourier model to the time-averaged
    spectrum, subtracts it and clips at ``sigma`` x MAD-of-MAD --
    ``tricolour.flagging.uvcontsub_flagger`` (flagging.py:989-1073), same
    arguments.  The reference is plain NumPy (float32 FFT / residuals under
    NumPy >= 2, float64 before); this follows the float32 semantics, so flags
    agree with it to within threshold-boundary cases, not bit for bit."""
    if tuple(vis.shape) != tuple(flags.shape):
        raise ValueError("vis and flags must have the same shape")       # flagging.py:1018-1019
    torch = _require_gpu()
    v, f8, code, from_numpy, device = _as_device_inputs(torch, vis, flags)
    if code != _lib.TRI_VIS_C64:
        raise TypeError("tricolour_amd.uvcontsub_flagger: visibilities must be complex64")
    f8 = _flags_u8(torch, flags, device)
    nbl, ncorr, ntime, nchan = (int(s) for s in v.shape)
    lib = _lib.lib()
    out = torch.empty(f8.shape, dtype=torch.uint8, device=device)
    n_cp = nbl * ncorr
    with torch.cuda.device(device):
        if n_cp > 0 and ntime > 0 and nchan > 0:
            # all windows go in one call: the library batches them itself, within the workspace it is handed
            _, nbytes = _window_batch(n_cp, lambda b: lib.tri_uvcontsub_workspace_bytes(b, ntime, nchan),
                                      lambda: _workspace_budget(torch, device), launch_cap=4096)
            ws = _workspace(torch, device, nbytes)
            _lib.check(lib.tri_uvcontsub_flagger(
                v.data_ptr(), f8.data_ptr(), out.data_ptr(), n_cp, ntime, nchan,
                int(major_cycles), int(or_original_from_cycle), int(taylor_degrees),
                float(sigma), ws.data_ptr(), ws.numel(),
                torch.cuda.current_stream(device).cuda_stream))
    return _like_flags(torch, out, flags, from_numpy)


def _sir(flags, missing, eta_time, eta_freq, penalty):
    """Both SIR calls: argument checks before any device work, then the library call (``missing is None``: the
    unmasked entry point), in window batches when the workspace does not fit the budget."""
    shape = tuple(flags.shape)
    if len(shape) != 4:
        raise ValueError("flags must be 4-D (bl, corr, time, chan), got shape %s" % (shape,))
    if missing is not None and tuple(missing.shape) != shape:
        raise ValueError("flags and missing must have the same shape, got %s and %s" % (shape, tuple(missing.shape)))
    eta_time, eta_freq = float(eta_time), float(eta_freq)
    for name, eta in (("eta_time", eta_time), ("eta_freq", eta_freq)):
        if not 0.0 <= eta < 1.0:              # also rejects NaN
            raise ValueError("%s must lie in [0, 1), got %r" % (name, eta))
    if missing is not None:
        penalty = float(penalty)
        if not 0.0 <= penalty < float("inf"):     # also rejects NaN
            raise ValueError("penalty must be finite and >= 0, got %r" % (penalty,))
    torch = _require_gpu()
    from_numpy = isinstance(flags, np.ndarray)
    device = flags.device if (torch.is_tensor(flags) and flags.is_cuda) else \
        torch.device("cuda", torch.cuda.current_device())
    f8 = _flags_u8(torch, flags, device)
    m8 = _flags_u8(torch, missing, device) if missing is not None else None
    nbl, ncorr, ntime, nchan = (int(s) for s in shape)
    n_win = nbl * ncorr
    out = torch.empty(f8.shape, dtype=torch.uint8, device=device)
    lib = _lib.lib()
    ws_bytes = lib.tri_sir_workspace_bytes if m8 is None else lib.tri_sir_masked_workspace_bytes
    with torch.cuda.device(device):
        if out.numel() > 0:
            # the workspace holds per-segment aggregates of lines longer than one workgroup; batch the windows
            # when even that does not fit (the only family without a launch cap)
            launches, tail = _window_launches(torch, device, n_win, lambda b: ws_bytes(b, ntime, nchan))
            for at, b in launches:
                if m8 is None:
                    _lib.check(lib.tri_scale_invariant_rank(at(f8), at(out), b, ntime, nchan, eta_time, eta_freq, *tail))
                else:
                    _lib.check(lib.tri_scale_invariant_rank_masked(at(f8), at(m8), at(out), b, ntime, nchan,
                                                                   eta_time, eta_freq, penalty, *tail))
    return _like_flags(torch, out, flags, from_numpy)


def scale_invariant_rank_operator(flags, eta_time=0.2, eta_freq=0.2):
    """Scale-invariant rank operator (Offringa, van de Gronde & Roerdink 2012,
    A&A 539, A95) on (bl, corr, time, chan) flags: a sample becomes flagged
    when some interval along time (``eta_time``) or frequency (``eta_freq``)
    that contains it has at most ``eta * length`` unflagged samples.  Both axes
    read the input mask: ``out = f | SIR_time(f) | SIR_freq(f)``; ``eta = 0``
    leaves an axis out.  Returns a new array in the container / dtype of
    ``flags``; the input is not modified."""
    return _sir(flags, None, eta_time, eta_freq, 0.0)


def scale_invariant_rank_operator_masked(flags, missing, eta_time=0.2, eta_freq=0.2, penalty=0.1):
    """:func:`scale_invariant_rank_operator` with a mask of missing samples
    (``missing``, shape of ``flags``, nonzero = missing): samples that are
    flagged without being detections -- absent cells of the window grid, dead
    samples, statically masked bands.  A present sample becomes flagged when
    some interval that contains it holds at most ``eta * (its present samples)
    - penalty * (its missing samples)`` present, unflagged samples: missing
    samples count neither as RFI nor as clean data, and crossing each costs
    ``penalty`` (0: flags on either side of a gap join freely; large: a gap is
    a wall).  A missing sample keeps its flag as it is.  ``out = f |
    SIRm_time(f, m) | SIRm_freq(f, m)``, both axes from the inputs; with no
    sample missing the result is :func:`scale_invariant_rank_operator`'s bit
    for bit.  Definition: ``include/tricolour_amd.h``.  Returns a new array in
    the container / dtype of ``flags``; the inputs are not modified."""
    if missing is None:
        raise ValueError("missing must be an array of the shape of flags")
    return _sir(flags, missing, eta_time, eta_freq, penalty)


def _line_rms_inputs(name, vis, flags):
    """Shape checks (before any device work) and device inputs of the line-RMS calls."""
    shape = tuple(vis.shape)
    if len(shape) != 4:
        raise ValueError("vis must be 4-D (bl, corr, time, chan), got shape %s" % (shape,))
    if tuple(flags.shape) != shape:
        raise ValueError("vis and flags must have the same shape, got %s and %s" % (shape, tuple(flags.shape)))
    torch = _require_gpu()
    v, _, code, from_numpy, device = _as_device_inputs(torch, vis, flags)
    if code not in (_lib.TRI_VIS_C64, _lib.TRI_VIS_F32):
        raise TypeError("tricolour_amd.%s: visibilities must be complex64 or float32" % name)
    return torch, v, _flags_u8(torch, flags, device), code, from_numpy, device


def _line_rms_cap(ntime, nchan):
    """Windows one launch of the line-RMS family holds (a launch holds 2^24 blocks: one per time row in the apply
    pass, one per 64 x 1024 tile in the power pass)."""
    tiles = -(-ntime // 64) * -(-nchan // 1024)
    return min(((1 << 24) - 1) // max(ntime, tiles), ((1 << 31) - 1) // (ntime + nchan))


def line_rms(vis, flags, _max_windows=None):
    """RMS of every time row (over channels) and of every channel (over times)
    of (bl, corr, time, chan) windows, over the unflagged, non-NaN samples:
    ``sqrt(sum |v|^2 / n)`` in float64 (float32 input: amplitudes).  Returns
    ``(rms_time (bl, corr, time), rms_chan (bl, corr, chan))``, NaN for lines
    without a counting sample -- numpy arrays for numpy input, tensors on the
    device otherwise.  The sums run in a fixed order: the same bits on every
    run and for every batch size.  Inputs are not modified."""
    torch, v, f8, code, from_numpy, device = _line_rms_inputs("line_rms", vis, flags)
    nbl, ncorr, ntime, nchan = (int(s) for s in v.shape)
    n_win = nbl * ncorr
    rms_t = torch.empty((nbl, ncorr, ntime), dtype=torch.float64, device=device)
    rms_c = torch.empty((nbl, ncorr, nchan), dtype=torch.float64, device=device)
    lib = _lib.lib()
    with torch.cuda.device(device):
        if v.numel() > 0:
            launches, tail = _window_launches(
                torch, device, n_win, lambda b: lib.tri_line_rms_workspace_bytes(b, ntime, nchan),
                _line_rms_cap(ntime, nchan), _max_windows)
            for at, b in launches:
                _lib.check(lib.tri_line_rms(at(v), code, at(f8), b, ntime, nchan, at(rms_t), at(rms_c), None, None, *tail))
    return _like_input(from_numpy, rms_t, rms_c)


def threshold_line_rms(vis, flags, nsigma_time=3.5, nsigma_freq=3.0, flag_low=True):
    """Flags whole timesteps and whole channels of (bl, corr, time, chan)
    windows on their RMS (after AOFlagger's ``threshold_timestep_rms`` /
    ``threshold_channel_rms``).  Per window and axis the line RMS values of
    :func:`line_rms` give ``med`` and ``sigma = 1.4826 * MAD``; a line is
    flagged when ``|rms - med| > nsigma * sigma`` (``flag_low=False``: only
    ``rms - med > nsigma * sigma``).  An axis with ``nsigma = 0``, with fewer
    than 3 finite lines or with ``sigma <= 1e-9 * med`` flags nothing, except
    that a line holding an unflagged infinite sample is always flagged when
    ``nsigma > 0``.  Both axes read the input flags:
    ``out = flags | bad_time | bad_chan``.  Returns a new array in the
    container / dtype of ``flags``; the inputs are not modified."""
    nsigma_time, nsigma_freq = float(nsigma_time), float(nsigma_freq)
    for name, ns in (("nsigma_time", nsigma_time), ("nsigma_freq", nsigma_freq)):
        if not ns >= 0.0:                     # also rejects NaN
            raise ValueError("%s must be >= 0, got %r" % (name, ns))
    torch, v, f8, code, from_numpy, device = _line_rms_inputs("threshold_line_rms", vis, flags)
    nbl, ncorr, ntime, nchan = (int(s) for s in v.shape)
    n_win = nbl * ncorr
    out = torch.empty(f8.shape, dtype=torch.uint8, device=device)
    lib = _lib.lib()
    with torch.cuda.device(device):
        if out.numel() > 0:
            launches, tail = _window_launches(
                torch, device, n_win, lambda b: lib.tri_line_rms_workspace_bytes(b, ntime, nchan),
                _line_rms_cap(ntime, nchan))
            for at, b in launches:
                _lib.check(lib.tri_line_rms_threshold(at(v), code, at(f8), at(out), b, ntime, nchan,
                                                      nsigma_time, nsigma_freq, 1 if flag_low else 0, *tail))
    return _like_flags(torch, out, flags, from_numpy)


def _ldev_window(name, w):
    """An odd integer in [3, 31], as an int (raises ValueError otherwise; bools and non-integral floats are not integers)."""
    try:
        ok = not isinstance(w, bool) and isinstance(w, (int, np.integer, float)) and float(w) == int(w)
    except (ValueError, OverflowError):       # NaN, infinity
        ok = False
    if not ok or int(w) % 2 == 0 or not 3 <= int(w) <= 31:
        raise ValueError("%s must be an odd integer in [3, 31], got %r" % (name, w))
    return int(w)


def _ldev_scale(name, s):
    try:
        ok = float(s) >= 0.0                  # also rejects NaN
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("%s must be >= 0, got %r" % (name, s))
    return float(s)


def _ldev_chunks(freq_chunks):
    ok = not isinstance(freq_chunks, bool) and isinstance(freq_chunks, (int, np.integer)) and int(freq_chunks) >= 1
    if not ok:
        raise ValueError("freq_chunks must be an integer >= 1, got %r" % (freq_chunks,))
    return int(freq_chunks)


def check_local_deviation_kwargs(window_time=3, window_freq=3, scale_time=3.5, scale_freq=3.5, freq_chunks=10):
    """The argument checks of :func:`threshold_local_deviation` (no device work): a window that is even or outside
    [3, 31], a scale that is negative or NaN and ``freq_chunks < 1`` raise ``ValueError``.  Returns the values."""
    return (_ldev_window("window_time", window_time), _ldev_window("window_freq", window_freq),
            _ldev_scale("scale_time", scale_time), _ldev_scale("scale_freq", scale_freq), _ldev_chunks(freq_chunks))


def _chunk_ends(nchan, freq_chunks):
    """The frequency chunk ends of the flagger (flagging.py:1172), as an array and as the library's int64 argument."""
    ends = np.linspace(0, nchan, freq_chunks + 1).astype(np.int64)
    return ends, (C.c_int64 * len(ends))(*[int(e) for e in ends])


def _ldev_cap(ntime, nchan, n_ends):
    """Windows one launch of the local-deviation family holds (every launch is one-dimensional and holds fewer than
    2^31 blocks: one per 8 rows x 1024 channels in the frequency pass, one per 4 (row, chunk) lines in its level
    pass, one per 256 samples in the scalar apply pass)."""
    lim = (1 << 31) - 1
    strips = -(-nchan // 1024)
    return min(lim // (ntime * strips), lim // -(-nchan // 32), lim // (ntime * (n_ends - 1)),
               lim // -(-(ntime * nchan) // 256))


def local_deviation(vis, flags, window_time=3, window_freq=3, _max_windows=None):
    """Sliding-window complex deviation of (bl, corr, time, chan) windows: for
    every sample the RMS of the complex deviations from their mean of the
    unflagged, non-NaN samples among the ``window`` samples around it, along
    time (``d_time``) and along frequency (``d_freq``), in float64 in a fixed
    order, stored as float32 (float32 input: amplitudes, ``im = 0``).  NaN
    where the sample itself does not count or fewer than 2 samples of its
    window do; ``+inf`` where a counting sample of the window has an infinite
    part.  Definition: ``include/tricolour_amd.h``.  Returns ``(d_time,
    d_freq)`` of the shape of ``vis`` -- numpy arrays for numpy input, tensors
    on the device otherwise.  Inputs are not modified."""
    window_time, window_freq = _ldev_window("window_time", window_time), _ldev_window("window_freq", window_freq)
    torch, v, f8, code, from_numpy, device = _line_rms_inputs("local_deviation", vis, flags)
    nbl, ncorr, ntime, nchan = (int(s) for s in v.shape)
    n_win = nbl * ncorr
    d_t = torch.empty(v.shape, dtype=torch.float32, device=device)
    d_f = torch.empty(v.shape, dtype=torch.float32, device=device)
    lib = _lib.lib()
    with torch.cuda.device(device):
        if v.numel() > 0:
            # batched as the thresholding call with one chunk (n_ends = 2), but the deviations alone take no workspace
            launches, (_, _, stream) = _window_launches(
                torch, device, n_win, lambda b: lib.tri_local_deviation_workspace_bytes(b, ntime, nchan, 2),
                _ldev_cap(ntime, nchan, 2), _max_windows, workspace=False)
            for at, b in launches:
                _lib.check(lib.tri_local_deviation(at(v), code, at(f8), b, ntime, nchan, window_time, window_freq,
                                                   at(d_t), at(d_f), stream))
    return _like_input(from_numpy, d_t, d_f)


def threshold_local_deviation(vis, flags, window_time=3, window_freq=3, scale_time=3.5, scale_freq=3.5, freq_chunks=10,
                              _max_windows=None):
    """Flags single samples of (bl, corr, time, chan) windows on the local
    deviation of the COMPLEX visibility (after CASA's ``rflag``; the definition
    is this library's own): :func:`local_deviation` gives ``d`` along each
    axis; per (window, channel) along time, and per (window, time row,
    frequency chunk) along frequency, the median ``med`` of the finite ``d`` is
    the level, and a usable sample is flagged when ``d > scale * med`` (or when
    ``d`` is ``+inf``).  A line with fewer than 3 finite values or ``med == 0``
    flags nothing else.  ``freq_chunks``: the frequency chunks of
    :func:`sum_threshold_flagger` (``linspace(0, nchan, freq_chunks + 1)``).
    Both axes read the inputs: ``out = flags | hit_time | hit_freq``; a scale
    of 0 switches an axis off.  Finds what the amplitude detectors cannot: a
    signal that scrambles the phase and leaves ``|v|`` alone.  Returns a new
    array in the container / dtype of ``flags``; the inputs are not modified."""
    window_time, window_freq, scale_time, scale_freq, freq_chunks = check_local_deviation_kwargs(
        window_time, window_freq, scale_time, scale_freq, freq_chunks)
    torch, v, f8, code, from_numpy, device = _line_rms_inputs("threshold_local_deviation", vis, flags)
    nbl, ncorr, ntime, nchan = (int(s) for s in v.shape)
    n_win = nbl * ncorr
    ends, ends_c = _chunk_ends(nchan, freq_chunks)
    out = torch.empty(f8.shape, dtype=torch.uint8, device=device)
    lib = _lib.lib()
    with torch.cuda.device(device):
        if out.numel() > 0:
            launches, tail = _window_launches(
                torch, device, n_win, lambda b: lib.tri_local_deviation_workspace_bytes(b, ntime, nchan, len(ends)),
                _ldev_cap(ntime, nchan, len(ends)), _max_windows)
            for at, b in launches:
                _lib.check(lib.tri_local_deviation_threshold(
                    at(v), code, at(f8), at(out), b, ntime, nchan, window_time, window_freq, scale_time, scale_freq,
                    ends_c, len(ends), *tail))
    return _like_flags(torch, out, flags, from_numpy)


HYST_MISSING = ("none", "input", "marked")     # the `missing` vocabulary of the strategy step (as the masked SIR step's)


def _hyst_reach(reach):
    ok = not isinstance(reach, bool) and isinstance(reach, (int, np.integer)) and 1 <= int(reach) <= 32
    if not ok:
        raise ValueError("reach must be an integer in [1, 32], got %r" % (reach,))
    return int(reach)


def check_hysteresis_kwargs(nsigma_time=2.5, nsigma_freq=2.5, reach=8, freq_chunks=10, missing="none"):
    """The argument checks of the ``hysteresis_growth`` step (no device work): an ``nsigma`` that is negative or NaN, a
    ``reach`` that is no integer in [1, 32], ``freq_chunks < 1`` and a ``missing`` other than ``none`` / ``input`` /
    ``marked`` raise ``ValueError``.  Returns the values."""
    if not isinstance(missing, str) or missing not in HYST_MISSING:
        raise ValueError("missing must be 'none', 'input' or 'marked', got %r" % (missing,))
    return (_ldev_scale("nsigma_time", nsigma_time), _ldev_scale("nsigma_freq", nsigma_freq), _hyst_reach(reach),
            _ldev_chunks(freq_chunks), missing)


def _hyst_cap(ntime, nchan, n_ends):
    """Windows one launch of the hysteresis family holds (every launch is one-dimensional and holds fewer than 2^31
    blocks: one per 8 channels and one per 4 (row, chunk) lines in the level passes, one per 8 rows x 256 channels in
    the eligibility pass)."""
    lim = (1 << 31) - 1
    return min(lim // -(-nchan // 8), (4 * lim) // (ntime * (n_ends - 1)) - 1, lim // (-(-ntime // 8) * -(-nchan // 256)))


def _hyst_launches(torch, lib, device, n_win, ntime, nchan, n_ends, max_windows):
    return _window_launches(torch, device, n_win, lambda b: lib.tri_hyst_workspace_bytes(b, ntime, nchan, n_ends),
                            _hyst_cap(ntime, nchan, n_ends), max_windows)


def robust_line_levels(vis, flags, freq_chunks=10, _max_windows=None):
    """Median and median absolute deviation of the amplitudes of every line of
    (bl, corr, time, chan) windows, over the unflagged samples with a finite
    amplitude: ``(med_t, mad_t)`` of shape (bl, corr, chan) for the lines along
    time, ``(med_f, mad_f)`` of shape (bl, corr, time, freq_chunks) for every
    time row's frequency chunks (``linspace(0, nchan, freq_chunks + 1)``).
    float32; ``mad`` is the median of ``fabsf(a - med)``; both are NaN where the
    line is not live (fewer than 3 samples, or a ``mad`` of 0).  The levels of
    :func:`hysteresis_growth`.  Returns numpy arrays for numpy input, tensors
    on the device otherwise.  Inputs are not modified."""
    freq_chunks = _ldev_chunks(freq_chunks)
    torch, v, f8, code, from_numpy, device = _line_rms_inputs("robust_line_levels", vis, flags)
    nbl, ncorr, ntime, nchan = (int(s) for s in v.shape)
    n_win = nbl * ncorr
    ends, ends_c = _chunk_ends(nchan, freq_chunks)
    nan = float("nan")
    lev = [torch.full((nbl, ncorr, nchan), nan, dtype=torch.float32, device=device) for _ in range(2)] + \
          [torch.full((nbl, ncorr, ntime, freq_chunks), nan, dtype=torch.float32, device=device) for _ in range(2)]
    lib = _lib.lib()
    with torch.cuda.device(device):
        if v.numel() > 0:
            launches, tail = _hyst_launches(torch, lib, device, n_win, ntime, nchan, len(ends), _max_windows)
            for at, b in launches:
                _lib.check(lib.tri_hyst_levels(at(v), code, at(f8), b, ntime, nchan, ends_c, len(ends),
                                               *(at(a) for a in lev), *tail))
    return _like_input(from_numpy, *lev)


def growth_eligibility(vis, flags, nsigma_time=2.5, nsigma_freq=2.5, freq_chunks=10, _max_windows=None):
    """The two eligibility images of :func:`hysteresis_growth`, bool, of the
    shape of ``vis``: ``e_time`` is set where an unflagged sample's amplitude
    exceeds ``med + nsigma_time * 1.4826 * mad`` of its (window, channel) line,
    ``e_freq`` the same with the levels of its (window, time row, frequency
    chunk); an unflagged ``+inf`` amplitude is eligible on every axis that is
    on, a NaN never.  ``nsigma = 0`` switches an axis off."""
    nsigma_time, nsigma_freq = _ldev_scale("nsigma_time", nsigma_time), _ldev_scale("nsigma_freq", nsigma_freq)
    freq_chunks = _ldev_chunks(freq_chunks)
    torch, v, f8, code, from_numpy, device = _line_rms_inputs("growth_eligibility", vis, flags)
    nbl, ncorr, ntime, nchan = (int(s) for s in v.shape)
    n_win = nbl * ncorr
    ends, ends_c = _chunk_ends(nchan, freq_chunks)
    e_t = torch.empty(f8.shape, dtype=torch.uint8, device=device)
    e_f = torch.empty(f8.shape, dtype=torch.uint8, device=device)
    lib = _lib.lib()
    with torch.cuda.device(device):
        if v.numel() > 0:
            launches, tail = _hyst_launches(torch, lib, device, n_win, ntime, nchan, len(ends), _max_windows)
            for at, b in launches:
                _lib.check(lib.tri_hyst_eligible(at(v), code, at(f8), b, ntime, nchan, nsigma_time, nsigma_freq,
                                                 ends_c, len(ends), at(e_t), at(e_f), *tail))
    e_t, e_f = e_t.view(torch.bool), e_f.view(torch.bool)
    return _like_input(from_numpy, e_t, e_f)


def grow_flags(seeds, e_time, e_freq, reach=8, _max_windows=None):
    """The growth rounds of :func:`hysteresis_growth` on any three images of
    shape (bl, corr, time, chan) (nonzero = set): ``G_0 = seeds`` and, ``reach``
    times, ``G |= (e_time & (G[t - 1] | G[t + 1])) | (e_freq & (G[c - 1] | G[c +
    1]))`` with every round reading the previous one and nothing beyond the
    window's edges.  A sample joins iff a path of at most ``reach`` steps leads
    to it from a seed through cells that are each eligible on the axis of the
    step taken.  Returns ``G_reach`` in the container / dtype of ``seeds``; the
    inputs are not modified."""
    reach = _hyst_reach(reach)
    shape = tuple(seeds.shape)
    if len(shape) != 4:
        raise ValueError("seeds must be 4-D (bl, corr, time, chan), got shape %s" % (shape,))
    for name, e in (("e_time", e_time), ("e_freq", e_freq)):
        if tuple(e.shape) != shape:
            raise ValueError("seeds and %s must have the same shape, got %s and %s" % (name, shape, tuple(e.shape)))
    torch = _require_gpu()
    from_numpy = isinstance(seeds, np.ndarray)
    device = seeds.device if (torch.is_tensor(seeds) and seeds.is_cuda) else \
        torch.device("cuda", torch.cuda.current_device())
    s8, t8, f8 = (_flags_u8(torch, a, device) for a in (seeds, e_time, e_freq))
    nbl, ncorr, ntime, nchan = (int(s) for s in shape)
    n_win = nbl * ncorr
    out = torch.empty(s8.shape, dtype=torch.uint8, device=device)
    lib = _lib.lib()
    with torch.cuda.device(device):
        if out.numel() > 0:
            launches, tail = _hyst_launches(torch, lib, device, n_win, ntime, nchan, 2, _max_windows)
            for at, b in launches:
                _lib.check(lib.tri_hyst_grow(at(s8), at(t8), at(f8), at(out), b, ntime, nchan, reach, *tail))
    return _like_flags(torch, out, seeds, from_numpy)


def hysteresis_growth(vis, flags, missing=None, nsigma_time=2.5, nsigma_freq=2.5, reach=8, freq_chunks=10,
                      _max_windows=None):
    """Value-driven growth of the flags of (bl, corr, time, chan) windows by
    two-level (hysteresis) thresholding (after the watershed of HERA's
    ``xrfi``; the definition is this library's own): what is flagged is a seed,
    and an unflagged neighbour along time (frequency) joins when its amplitude
    exceeds ``med + nsigma * 1.4826 * mad`` of its (window, channel) line (its
    (window, time row, frequency chunk) line) -- see :func:`robust_line_levels`
    and :func:`growth_eligibility`.  ``reach`` synchronous rounds
    (:func:`grow_flags`): a sample joins iff a path of at most ``reach`` steps
    leads to it from a seed through cells that are each eligible on the axis of
    the step taken.  ``missing`` (shape of ``flags``, nonzero = missing, or
    None): flagged samples that are no detections; they seed nothing and, being
    flagged, block growth.  ``nsigma = 0`` switches an axis off.  ``out = flags
    | G_reach``.  Definition: ``include/tricolour_amd.h``.  Returns a new array
    in the container / dtype of ``flags``; the inputs are not modified."""
    nsigma_time, nsigma_freq, reach, freq_chunks, _ = check_hysteresis_kwargs(nsigma_time, nsigma_freq, reach, freq_chunks)
    if missing is not None and tuple(missing.shape) != tuple(flags.shape):
        raise ValueError("flags and missing must have the same shape, got %s and %s"
                         % (tuple(flags.shape), tuple(missing.shape)))
    torch, v, f8, code, from_numpy, device = _line_rms_inputs("hysteresis_growth", vis, flags)
    m8 = _flags_u8(torch, missing, device) if missing is not None else None
    nbl, ncorr, ntime, nchan = (int(s) for s in v.shape)
    n_win = nbl * ncorr
    ends, ends_c = _chunk_ends(nchan, freq_chunks)
    out = torch.empty(f8.shape, dtype=torch.uint8, device=device)
    lib = _lib.lib()
    with torch.cuda.device(device):
        if out.numel() > 0:
            launches, tail = _hyst_launches(torch, lib, device, n_win, ntime, nchan, len(ends), _max_windows)
            for at, b in launches:
                _lib.check(lib.tri_hysteresis_growth(at(v), code, at(f8), at(m8), at(out), b, ntime, nchan,
                                                     nsigma_time, nsigma_freq, reach, ends_c, len(ends), *tail))
    return _like_flags(torch, out, flags, from_numpy)


MEDZ_MAX_RADIUS = 32        # largest radius of the sliding median
MEDZ_MAX_AREA = 625         # largest neighbourhood, (2 radius_time + 1) (2 radius_freq + 1)
MEDZ_MAX_ROUNDS = 4


def _medz_int(name, v):
    """An integer as an int, or None (bools and non-integral floats are not integers)."""
    try:
        ok = not isinstance(v, bool) and isinstance(v, (int, np.integer, float)) and float(v) == int(v)
    except (ValueError, OverflowError):       # NaN, infinity
        ok = False
    return int(v) if ok else None


def _medz_radii(radius_time, radius_freq, min_samples):
    kt, kf = _medz_int("radius_time", radius_time), _medz_int("radius_freq", radius_freq)
    for name, k, given in (("radius_time", kt, radius_time), ("radius_freq", kf, radius_freq)):
        if k is None or not 0 <= k <= MEDZ_MAX_RADIUS:
            raise ValueError("%s must be an integer in [0, %d], got %r" % (name, MEDZ_MAX_RADIUS, given))
    if kt == 0 and kf == 0:
        raise ValueError("radius_time and radius_freq must not both be 0")
    area = (2 * kt + 1) * (2 * kf + 1)
    if area > MEDZ_MAX_AREA:
        raise ValueError("(2 radius_time + 1) (2 radius_freq + 1) must be at most %d, got %d" % (MEDZ_MAX_AREA, area))
    if min_samples is None:
        ms = max(1, (area + 7) // 8)
    else:
        ms = _medz_int("min_samples", min_samples)
        if ms is None or not 1 <= ms <= area:
            raise ValueError("min_samples must be an integer in [1, %d], got %r" % (area, min_samples))
    return kt, kf, ms


def check_median_zscore_kwargs(nsigma=6.0, radius_time=8, radius_freq=8, min_samples=None, rounds=1):
    """The argument checks of :func:`threshold_median_zscore` (no device work): a radius that is no integer in
    [0, 32], both radii 0, a neighbourhood of more than 625 samples, ``min_samples`` outside [1, neighbourhood],
    ``nsigma`` that is not > 0 and ``rounds`` outside [1, 4] raise ``ValueError``.  Returns the values, ``min_samples``
    resolved (``None``: an eighth of the neighbourhood, rounded up, at least 1)."""
    try:
        ok = float(nsigma) > 0.0              # also rejects NaN
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("nsigma must be > 0, got %r" % (nsigma,))
    kt, kf, ms = _medz_radii(radius_time, radius_freq, min_samples)
    r = _medz_int("rounds", rounds)
    if r is None or not 1 <= r <= MEDZ_MAX_ROUNDS:
        raise ValueError("rounds must be an integer in [1, %d], got %r" % (MEDZ_MAX_ROUNDS, rounds))
    return float(nsigma), kt, kf, ms, r


def _medz_inputs(name, vis, flags):
    """Shape and dtype checks (ValueError, before any device work) and device inputs of the median z-score calls."""
    shape = tuple(vis.shape)
    if len(shape) != 4:
        raise ValueError("vis must be 4-D (bl, corr, time, chan), got shape %s" % (shape,))
    if tuple(flags.shape) != shape:
        raise ValueError("vis and flags must have the same shape, got %s and %s" % (shape, tuple(flags.shape)))
    if str(vis.dtype).replace("torch.", "") not in ("complex64", "float32"):
        raise ValueError("tricolour_amd.%s: visibilities must be complex64 or float32, got %s" % (name, vis.dtype))
    return _line_rms_inputs(name, vis, flags)


def _medz_cap(ntime, nchan):
    """Windows one launch of the median z-score family holds (every launch is one-dimensional and holds fewer than
    2^31 blocks: one per tile of 16 rows x 64 channels)."""
    return ((1 << 31) - 1) // (-(-ntime // 16) * -(-nchan // 64))


def _medz_launches(torch, device, n_win, ntime, nchan, max_windows):
    """The batches of a median z-score call, sized so that two float32 images of a batch (8 bytes per sample: the
    residual and the z-score) fit the workspace budget, as a list of ``(at, b)``, and the stream."""
    launches, (_, _, stream) = _window_launches(torch, device, n_win, lambda b: 8 * b * ntime * nchan,
                                                _medz_cap(ntime, nchan), max_windows, workspace=False)
    return list(launches), stream


def median_filter_background(vis, flags, radius_time=8, radius_freq=8, min_samples=None, _max_windows=None):
    """Sliding 2-D median background of (bl, corr, time, chan) windows (after
    ``detrend_medfilt`` of HERA's ``xrfi``; the definition is this library's
    own): ``background`` is, at EVERY sample, the median amplitude of the
    unflagged, finite samples within ``radius_time`` rows and ``radius_freq``
    channels of it, the neighbourhood cut at the window's edges; NaN where
    fewer than ``min_samples`` count (``None``: an eighth of the neighbourhood).
    ``residual = amplitude - background`` where the sample itself counts and
    the background is defined, NaN elsewhere.  A robust bandpass / waterfall:
    defined under flags too, and one pass, since the median ignores what is not
    yet flagged.  Definition: ``include/tricolour_amd.h``.  Returns
    ``(background, residual)``, float32 of the shape of ``vis`` -- numpy arrays
    for numpy input, tensors on the device otherwise.  Inputs are not
    modified."""
    kt, kf, ms = _medz_radii(radius_time, radius_freq, min_samples)
    torch, v, f8, code, from_numpy, device = _medz_inputs("median_filter_background", vis, flags)
    nbl, ncorr, ntime, nchan = (int(s) for s in v.shape)
    n_win = nbl * ncorr
    bg = torch.empty(v.shape, dtype=torch.float32, device=device)
    res = torch.empty(v.shape, dtype=torch.float32, device=device)
    lib = _lib.lib()
    with torch.cuda.device(device):
        if v.numel() > 0:
            launches, stream = _medz_launches(torch, device, n_win, ntime, nchan, _max_windows)
            for at, b in launches:
                _lib.check(lib.tri_medfilt_background(at(v), code, at(f8), b, ntime, nchan, kt, kf, ms, at(bg), at(res),
                                                      stream))
    return _like_input(from_numpy, bg, res)


def median_zscore(vis, flags, radius_time=8, radius_freq=8, min_samples=None, _max_windows=None):
    """Robust (modified) z-score of (bl, corr, time, chan) windows against
    their sliding median background: with ``residual`` of
    :func:`median_filter_background`, ``scale`` is the sliding median, over the
    same neighbourhood and by the same rule, of ``|residual|`` and ``z =
    residual / (1.4826 * scale)`` in float64, stored as float32; NaN where the
    residual or the scale is.  Definition: ``include/tricolour_amd.h``.  Returns
    ``z`` of the shape of ``vis`` -- a numpy array for numpy input, a tensor on
    the device otherwise.  ``z`` is a float32 image like any other: the steps
    that take float32 amplitudes accept it.  Inputs are not modified."""
    kt, kf, ms = _medz_radii(radius_time, radius_freq, min_samples)
    torch, v, f8, code, from_numpy, device = _medz_inputs("median_zscore", vis, flags)
    nbl, ncorr, ntime, nchan = (int(s) for s in v.shape)
    n_win = nbl * ncorr
    z = torch.empty(v.shape, dtype=torch.float32, device=device)
    lib = _lib.lib()
    with torch.cuda.device(device):
        if v.numel() > 0:
            launches, stream = _medz_launches(torch, device, n_win, ntime, nchan, _max_windows)
            # the residual of one batch at a time; its background passes through the batch's part of z
            res = torch.empty((launches[0][1], ntime, nchan), dtype=torch.float32, device=device)
            for at, b in launches:
                _lib.check(lib.tri_medfilt_background(at(v), code, at(f8), b, ntime, nchan, kt, kf, ms, at(z),
                                                      res.data_ptr(), stream))
                _lib.check(lib.tri_medfilt_zscore(res.data_ptr(), b, ntime, nchan, kt, kf, ms, None, at(z), stream))
    return _like_input(from_numpy, z)[0]


def threshold_median_zscore(vis, flags, nsigma=6.0, radius_time=8, radius_freq=8, min_samples=None, rounds=1,
                            _max_windows=None):
    """Flags single samples of (bl, corr, time, chan) windows on their robust
    z-score against a sliding 2-D median background (after ``detrend_medfilt``
    of HERA's ``xrfi``; the definition is this library's own): a sample is hit
    when ``|z| > nsigma`` with ``z`` of :func:`median_zscore`.  Background and
    scale are local -- ``radius_time`` rows and ``radius_freq`` channels around
    the sample -- and medians, so interference that is not yet flagged does not
    pull them up and one round does what the linear background needs
    iterations for.  ``rounds`` > 1 repeats the step on the grown flags:
    ``g_k = g_{k-1} | hits(vis, g_{k-1})``.  ``out = flags | hits``.
    Definition: ``include/tricolour_amd.h``.  Returns a new array in the
    container / dtype of ``flags``; the inputs are not modified."""
    nsigma, kt, kf, ms, rounds = check_median_zscore_kwargs(nsigma, radius_time, radius_freq, min_samples, rounds)
    torch, v, f8, code, from_numpy, device = _medz_inputs("threshold_median_zscore", vis, flags)
    nbl, ncorr, ntime, nchan = (int(s) for s in v.shape)
    n_win = nbl * ncorr
    out = torch.empty(f8.shape, dtype=torch.uint8, device=device)
    lib = _lib.lib()
    with torch.cuda.device(device):
        if out.numel() > 0:
            launches, stream = _medz_launches(torch, device, n_win, ntime, nchan, _max_windows)
            # the library's two output images of one batch at a time
            res = torch.empty((launches[0][1], ntime, nchan), dtype=torch.float32, device=device)
            z = torch.empty_like(res)
            for at, b in launches:
                _lib.check(lib.tri_median_zscore_threshold(at(v), code, at(f8), at(out), b, ntime, nchan, kt, kf, ms,
                                                           nsigma, rounds, res.data_ptr(), z.data_ptr(), stream))
    return _like_flags(torch, out, flags, from_numpy)


SK_MAX_BLOCK = 65536        # largest block_time of the spectral-kurtosis step


def _sk_block(block_time):
    m = _medz_int("block_time", block_time)
    if m is None or not 2 <= m <= SK_MAX_BLOCK:
        raise ValueError("block_time must be an integer in [2, %d], got %r" % (SK_MAX_BLOCK, block_time))
    return m


def _sk_nsigma(name, v):
    """``None`` (the side is off) or a float > 0."""
    if v is None:
        return None
    try:
        ok = not isinstance(v, bool) and 0.0 < float(v) < float("inf")       # also rejects NaN
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("%s must be None or a finite number > 0, got %r" % (name, v))
    return float(v)


def _sk_params(block_time, shape, min_samples):
    m = _sk_block(block_time)
    try:
        ok = not isinstance(shape, bool) and 0.0 < float(shape) < float("inf")    # also rejects NaN
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("shape must be a finite number > 0, got %r" % (shape,))
    if min_samples is None:
        ms = max(2, m // 2)
    else:
        ms = _medz_int("min_samples", min_samples)
        if ms is None or not 2 <= ms <= m:
            raise ValueError("min_samples must be an integer in [2, %d], got %r" % (m, min_samples))
    return m, float(shape), ms


def check_spectral_kurtosis_kwargs(block_time=64, shape=1.0, min_samples=None, nsigma_low=4.0, nsigma_high=4.0):
    """The argument checks of :func:`threshold_spectral_kurtosis` (no device work): ``block_time`` that is no integer in
    [2, 65536], ``shape`` that is not a finite number > 0, ``min_samples`` that is no integer in [2, block_time] and an
    ``nsigma_low`` / ``nsigma_high`` that is neither ``None`` nor a finite number > 0 raise ``ValueError`` naming the
    argument; booleans are no numbers here.  Returns the values, ``min_samples`` resolved (``None``: half a block, at
    least 2)."""
    m, d, ms = _sk_params(block_time, shape, min_samples)
    return m, d, ms, _sk_nsigma("nsigma_low", nsigma_low), _sk_nsigma("nsigma_high", nsigma_high)


def spectral_kurtosis_bounds(block_time, shape=1.0, nsigma_low=4.0, nsigma_high=4.0):
    """The default decision tables of the spectral-kurtosis step, ``(lower, upper)``: ``block_time + 1`` float64
    each, indexed by a cell's valid count ``n``.  With ``d = shape``, for ``n >= 2``:
    ``sigma(n) = sqrt(2 d (d + 1) n^2 / ((n - 1)(n d + 2)(n d + 3)))`` (the estimator's standard deviation under a
    gamma law of shape ``d``), ``lower[n] = exp(-nsigma_low * sigma(n))`` and ``upper[n] = exp(+nsigma_high *
    sigma(n))``: symmetric in ``ln sk``, as the estimator's skewed distribution nearly is, not in ``sk``.  The entries
    for ``n < 2`` are NaN, and a side given as ``None`` is NaN throughout: a NaN entry never hits.  Host arithmetic in
    NumPy float64."""
    m, d, _, lo, hi = check_spectral_kurtosis_kwargs(block_time, shape, None, nsigma_low, nsigma_high)
    n = np.arange(m + 1, dtype=np.float64)
    lower = np.full(m + 1, np.nan)
    upper = np.full(m + 1, np.nan)
    k = n[2:]
    sigma = np.sqrt(2.0 * d * (d + 1.0) * k * k / ((k - 1.0) * (k * d + 2.0) * (k * d + 3.0)))
    if lo is not None:
        lower[2:] = np.exp(-lo * sigma)
    if hi is not None:
        upper[2:] = np.exp(hi * sigma)
    return lower, upper


def _sk_tables(bounds, m):
    """``bounds = (lower, upper)`` as two float64 arrays of ``m + 1`` entries (any values: NaN switches an entry off)."""
    try:
        lower, upper = bounds
        lower, upper = np.array(lower, np.float64), np.array(upper, np.float64)
    except (TypeError, ValueError):
        raise ValueError("bounds must be a pair (lower, upper) of arrays of numbers") from None
    for name, t in (("lower", lower), ("upper", upper)):
        if t.shape != (m + 1,):
            raise ValueError("bounds: %s must hold block_time + 1 = %d entries, got shape %s" % (name, m + 1, t.shape))
    return lower, upper


def _sk_cap(ntime, nchan, m):
    """Windows one launch of the spectral-kurtosis family holds (every launch is one-dimensional and holds fewer than
    2^31 blocks; the apply pass has the most: one per block of rows, 16 rows of it and 256 channels)."""
    return ((1 << 31) - 1) // (-(-ntime // m) * -(-m // 16) * -(-nchan // 256))


def _sk_launches(torch, device, n_win, ntime, nchan, m, max_windows):
    """The batches of a spectral-kurtosis call (there is no workspace to size them against) as a list of ``(at, b)``,
    and the stream."""
    launches, (_, _, stream) = _window_launches(torch, device, n_win, lambda b: 0, _sk_cap(ntime, nchan, m),
                                                max_windows, workspace=False)
    return list(launches), stream


def spectral_kurtosis(vis, flags, block_time=64, shape=1.0, min_samples=None, _max_windows=None):
    """Spectral kurtosis (Nita & Gary 2010) of (bl, corr, time, chan) windows
    over tiled blocks of ``block_time`` rows: per block and channel, with ``n``
    the number of unflagged, finite samples and ``S1``, ``S2`` the sums of their
    powers and squared powers (float64, rows in ascending order),
    ``sk = ((n d + 1) / (n - 1)) (n S2 / S1^2 - 1)`` with ``d = shape``: 1 for
    raw correlator dumps, N for data that is already an average of N.  Its
    expectation on noise is 1 whatever the level; pulsed interference pushes it
    up, a steady carrier towards 0.  NaN where ``n < min_samples`` (``None``:
    half a block) or the powers sum to 0.  Definition:
    ``include/tricolour_amd.h``.  Returns ``(sk float32, count int32)`` of shape
    (bl, corr, ceil(time / block_time), chan) -- numpy arrays for numpy input,
    tensors on the device otherwise.  Inputs are not modified."""
    m, d, ms = _sk_params(block_time, shape, min_samples)
    torch, v, f8, code, from_numpy, device = _medz_inputs("spectral_kurtosis", vis, flags)
    nbl, ncorr, ntime, nchan = (int(s) for s in v.shape)
    n_win = nbl * ncorr
    nb = -(-ntime // m)
    sk = torch.empty((nbl, ncorr, nb, nchan), dtype=torch.float32, device=device)
    cnt = torch.empty((nbl, ncorr, nb, nchan), dtype=torch.int32, device=device)
    lib = _lib.lib()
    with torch.cuda.device(device):
        if v.numel() > 0:
            launches, stream = _sk_launches(torch, device, n_win, ntime, nchan, m, _max_windows)
            for at, b in launches:
                _lib.check(lib.tri_sk_statistics(at(v), code, at(f8), b, ntime, nchan, m, d, ms, at(sk), at(cnt), stream))
    return _like_input(from_numpy, sk, cnt)


def apply_spectral_kurtosis(sk, count, flags, block_time, bounds, _max_windows=None):
    """Flags whole (block, channel) cells on statistics of
    :func:`spectral_kurtosis`: with ``bounds = (lower, upper)``, two tables of
    ``block_time + 1`` numbers indexed by a cell's count ``n`` (the defaults:
    :func:`spectral_kurtosis_bounds`; Pearson-type or Monte-Carlo bounds go in
    the same way), a cell is hit when ``sk < lower[n]`` or ``sk > upper[n]``.
    A NaN ``sk`` and a NaN table entry never hit.  ``out[.., t, f] = flags[..,
    t, f] | hit[.., t // block_time, f]``.  ``sk`` float32 and ``count`` int32
    of shape (bl, corr, ceil(time / block_time), chan), ``flags`` (bl, corr,
    time, chan).  Returns a new array in the container / dtype of ``flags``;
    the inputs are not modified."""
    m = _sk_block(block_time)
    lower, upper = _sk_tables(bounds, m)
    shape = tuple(flags.shape)
    if len(shape) != 4:
        raise ValueError("flags must be 4-D (bl, corr, time, chan), got shape %s" % (shape,))
    cells = (shape[0], shape[1], -(-shape[2] // m), shape[3])
    for name, a, dt in (("sk", sk, "float32"), ("count", count, "int32")):
        if tuple(a.shape) != cells:
            raise ValueError("%s must have the shape %s, got %s" % (name, cells, tuple(a.shape)))
        if str(a.dtype).replace("torch.", "") != dt:
            raise ValueError("%s must be %s, got %s" % (name, dt, a.dtype))
    torch = _require_gpu()
    from_numpy = any(isinstance(a, np.ndarray) for a in (sk, count, flags))
    device = next((a.device for a in (flags, sk, count) if torch.is_tensor(a) and a.is_cuda),
                  torch.device("cuda", torch.cuda.current_device()))
    f8 = _flags_u8(torch, flags, device)
    s, c = (_sk_dev(torch, device, a) for a in (sk, count))
    nbl, ncorr, ntime, nchan = (int(x) for x in shape)
    n_win = nbl * ncorr
    out = torch.empty(f8.shape, dtype=torch.uint8, device=device)
    lib = _lib.lib()
    with torch.cuda.device(device):
        if out.numel() > 0:
            lo, hi = _sk_dev(torch, device, lower), _sk_dev(torch, device, upper)
            launches, stream = _sk_launches(torch, device, n_win, ntime, nchan, m, _max_windows)
            for at, b in launches:
                _lib.check(lib.tri_sk_apply(at(s), at(c), at(f8), at(out), b, ntime, nchan, m, lo.data_ptr(),
                                            hi.data_ptr(), stream))
    return _like_flags(torch, out, flags, from_numpy)


def _sk_dev(torch, device, a):
    """A contiguous device tensor of a numpy array or tensor."""
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a))
    return a.to(device).contiguous()


def threshold_spectral_kurtosis(vis, flags, block_time=64, shape=1.0, min_samples=None, nsigma_low=4.0, nsigma_high=4.0,
                                bounds=None, _max_windows=None):
    """Flags whole (block of ``block_time`` rows, channel) cells of (bl, corr,
    time, chan) windows whose spectral kurtosis (:func:`spectral_kurtosis`) is
    not that of noise: above ``upper[n]`` -- pulsed or intermittent
    interference, too sparse for the SumThreshold windows and too weak for a
    line RMS -- or below ``lower[n]`` -- a steady carrier, which a background
    fit absorbs as level.  No background, noise estimate or bandpass enters.
    The tables are :func:`spectral_kurtosis_bounds` of ``nsigma_low`` /
    ``nsigma_high`` (``None`` switches a side off), or ``bounds = (lower,
    upper)`` in their place.  ``out = flags | hits``; a second round could not
    change anything.  Where a bright source's fringe dominates the noise within
    a block the estimator reads low without any interference: apply the step to
    noise-dominated data (residuals), or with ``nsigma_low=None``.  Definition:
    ``include/tricolour_amd.h``.  Returns a new array in the container / dtype
    of ``flags``; the inputs are not modified."""
    m, d, ms, lo, hi = check_spectral_kurtosis_kwargs(block_time, shape, min_samples, nsigma_low, nsigma_high)
    lower, upper = spectral_kurtosis_bounds(m, d, lo, hi) if bounds is None else _sk_tables(bounds, m)
    torch, v, f8, code, from_numpy, device = _medz_inputs("threshold_spectral_kurtosis", vis, flags)
    nbl, ncorr, ntime, nchan = (int(s) for s in v.shape)
    n_win = nbl * ncorr
    out = torch.empty(f8.shape, dtype=torch.uint8, device=device)
    lib = _lib.lib()
    with torch.cuda.device(device):
        if out.numel() > 0:
            lo_t, hi_t = _sk_dev(torch, device, lower), _sk_dev(torch, device, upper)
            launches, stream = _sk_launches(torch, device, n_win, ntime, nchan, m, _max_windows)
            # the library's two statistics images of one batch at a time
            sk = torch.empty((launches[0][1], -(-ntime // m), nchan), dtype=torch.float32, device=device)
            cnt = torch.empty(sk.shape, dtype=torch.int32, device=device)
            for at, b in launches:
                _lib.check(lib.tri_sk_threshold(at(v), code, at(f8), at(out), b, ntime, nchan, m, d, ms, lo_t.data_ptr(),
                                                hi_t.data_ptr(), sk.data_ptr(), cnt.data_ptr(), stream))
    return _like_flags(torch, out, flags, from_numpy)


PF_ORDERS = ("freqtime", "timefreq", "freq", "time")    # the `order` vocabulary of the polynomial-fit step, by ABI code
PF_AXES = ("time", "freq")                              # the `axis` vocabulary of its background call, by ABI code
PF_MAX_PIECES = 32
PF_MAX_ROUNDS = 16
PF_MAX_LINE = 16384         # longest fitted line, either axis


def _pf_int(name, v, lo, hi):
    k = _medz_int(name, v)
    if k is None or not lo <= k <= hi:
        raise ValueError("%s must be an integer in [%d, %d], got %r" % (name, lo, hi, v))
    return k


def _pf_cutoff(name, v):
    try:
        ok = not isinstance(v, bool) and 0.0 < float(v) < float("inf")       # also rejects NaN
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("%s must be a finite number > 0, got %r" % (name, v))
    return float(v)


def check_polyfit_kwargs(order="freqtime", time_cutoff=4.0, time_degree=1, time_pieces=1, freq_cutoff=3.0, freq_degree=3,
                         freq_pieces=7, rounds=5, min_samples=8):
    """The argument checks of :func:`threshold_polyfit` (no device work): an ``order`` outside ``freqtime``,
    ``timefreq``, ``freq``, ``time``, a cutoff that is not a finite number > 0, a degree that is no integer in [0, 3],
    pieces outside [1, 32], ``rounds`` outside [1, 16] and ``min_samples`` that is no integer >= 2 raise ``ValueError``
    naming the argument; booleans are no numbers here.  Returns the values in the order of the arguments."""
    if not isinstance(order, str) or order not in PF_ORDERS:
        raise ValueError("order must be one of %s, got %r" % (", ".join(PF_ORDERS), order))
    return (order, _pf_cutoff("time_cutoff", time_cutoff), _pf_int("time_degree", time_degree, 0, 3),
            _pf_int("time_pieces", time_pieces, 1, PF_MAX_PIECES), _pf_cutoff("freq_cutoff", freq_cutoff),
            _pf_int("freq_degree", freq_degree, 0, 3), _pf_int("freq_pieces", freq_pieces, 1, PF_MAX_PIECES),
            _pf_int("rounds", rounds, 1, PF_MAX_ROUNDS), _pf_int("min_samples", min_samples, 2, (1 << 31) - 1))


def _pf_cap(ntime, nchan):
    """Windows one launch of the polynomial-fit family holds (every launch is one-dimensional and holds fewer than
    2^31 blocks: one per time row in the frequency pass, one per 256 samples in the prepare and finish passes)."""
    return ((1 << 31) - 1) // (ntime * -(-nchan // 256))


def _pf_line_limit(shape, time, freq):
    """The library's limit on a fitted line, from the input's shape alone: raised before any device work (a shape that is
    not 4-D is left to the input checks)."""
    if len(shape) != 4:
        return
    ntime, nchan = int(shape[2]), int(shape[3])
    if (time and ntime > PF_MAX_LINE) or (freq and nchan > PF_MAX_LINE):
        raise NotImplementedError("a fitted line holds at most %d samples, got %d times and %d channels"
                                  % (PF_MAX_LINE, ntime, nchan))


def polyfit_background(vis, flags, axis="freq", pieces=1, degree=3, _max_windows=None):
    """Piecewise-polynomial fit along every line of one axis of (bl, corr, time,
    chan) windows: ``axis="freq"`` fits each time row over its channels (a
    bandpass), ``axis="time"`` each channel over its rows (a time trend).  The
    line is cut into ``pieces`` equal pieces, each fitted by least squares with
    a polynomial of ``degree`` (0..3) to the amplitudes of its unflagged,
    finite samples; a piece whose samples cannot carry the degree gets a lower
    one, down to the mean.  Returns the fit as float32 of the shape of ``vis``,
    evaluated at EVERY sample, flagged ones included, NaN where a piece holds
    no usable sample -- a numpy array for numpy input, a tensor on the device
    otherwise.  One fit, no rejection: call it with the flags of
    :func:`threshold_polyfit` for the robust curve.  Definition:
    ``include/tricolour_amd.h``.  Lines of more than 16384 samples raise
    ``NotImplementedError``.  Inputs are not modified."""
    if not isinstance(axis, str) or axis not in PF_AXES:
        raise ValueError("axis must be one of %s, got %r" % (", ".join(PF_AXES), axis))
    pieces = _pf_int("pieces", pieces, 1, PF_MAX_PIECES)
    degree = _pf_int("degree", degree, 0, 3)
    time = axis == "time"
    _pf_line_limit(tuple(vis.shape), time, not time)
    torch, v, f8, code, from_numpy, device = _medz_inputs("polyfit_background", vis, flags)
    nbl, ncorr, ntime, nchan = (int(s) for s in v.shape)
    n_win = nbl * ncorr
    bg = torch.empty(v.shape, dtype=torch.float32, device=device)
    lib = _lib.lib()
    tp = pieces if time else 0
    with torch.cuda.device(device):
        if v.numel() > 0:
            launches, tail = _window_launches(
                torch, device, n_win, lambda b: lib.tri_polyfit_workspace_bytes(b, ntime, nchan, tp), _pf_cap(ntime, nchan),
                _max_windows)
            for at, b in launches:
                _lib.check(lib.tri_polyfit_background(at(v), code, at(f8), b, ntime, nchan, PF_AXES.index(axis), pieces,
                                                      degree, at(bg), *tail))
    return _like_input(from_numpy, bg)[0]


def threshold_polyfit(vis, flags, order="freqtime", time_cutoff=4.0, time_degree=1, time_pieces=1, freq_cutoff=3.0,
                      freq_degree=3, freq_pieces=7, rounds=5, min_samples=8, _max_windows=None):
    """Flags single samples of (bl, corr, time, chan) windows that stand off a
    robust piecewise-polynomial fit along their line (after CASA's ``tfcrop``;
    the definition is this library's own).  Every line is normalised by itself:
    the fit absorbs a bandpass shape, a fringe or a gain drift, and the
    threshold is the scatter about the fit on the same line, so it works on
    uncalibrated data.  Per line, ``rounds`` rounds: fit the samples not yet
    hit -- a straight line over the whole line first, then ``min(2 r + 1,
    pieces)`` pieces of ``degree`` -- and hit those whose residual exceeds
    ``cutoff`` times the RMS residual of the round.  Lines with fewer than
    ``min_samples`` usable samples are left alone.  ``order``: ``"freqtime"``
    (along frequency, then along time on what is left), ``"timefreq"``,
    ``"freq"`` or ``"time"``.  ``out = flags | hits``.  Definition:
    ``include/tricolour_amd.h``.  Lines of more than 16384 samples along a
    fitted axis raise ``NotImplementedError``.  Returns a new array in the
    container / dtype of ``flags``; the inputs are not modified."""
    order, ct, dt, pt, cf, df, pf, rounds, ms = check_polyfit_kwargs(
        order, time_cutoff, time_degree, time_pieces, freq_cutoff, freq_degree, freq_pieces, rounds, min_samples)
    _pf_line_limit(tuple(vis.shape), order != "freq", order != "time")
    torch, v, f8, code, from_numpy, device = _medz_inputs("threshold_polyfit", vis, flags)
    nbl, ncorr, ntime, nchan = (int(s) for s in v.shape)
    n_win = nbl * ncorr
    out = torch.empty(f8.shape, dtype=torch.uint8, device=device)
    lib = _lib.lib()
    with torch.cuda.device(device):
        if out.numel() > 0:
            launches, tail = _window_launches(
                torch, device, n_win, lambda b: lib.tri_polyfit_workspace_bytes(b, ntime, nchan, pt),
                _pf_cap(ntime, nchan), _max_windows)
            for at, b in launches:
                _lib.check(lib.tri_polyfit_threshold(at(v), code, at(f8), at(out), b, ntime, nchan, PF_ORDERS.index(order),
                                                     ct, dt, pt, cf, df, pf, rounds, ms, *tail))
    return _like_flags(torch, out, flags, from_numpy)


def _bli_inputs(name, vis, flags, select):
    """Checks of the baseline-integration calls (all before any device work), then the device inputs:
    (torch, vis, flags uint8, dtype code, from_numpy, device, select uint8 on the device or None)."""
    shape = tuple(vis.shape)
    if len(shape) != 4:
        raise ValueError("vis must be 4-D (bl, corr, time, chan), got shape %s" % (shape,))
    if tuple(flags.shape) != shape:
        raise ValueError("vis and flags must have the same shape, got %s and %s" % (shape, tuple(flags.shape)))
    if str(vis.dtype).replace("torch.", "") not in ("complex64", "float32"):
        raise TypeError("tricolour_amd.%s: visibilities must be complex64 or float32 (got %s)" % (name, vis.dtype))
    if select is not None:
        if not hasattr(select, "shape"):
            select = np.asarray(select)
        if tuple(select.shape) != (shape[0],):
            raise ValueError("select must have one entry per baseline (%d), got shape %s"
                             % (shape[0], tuple(select.shape)))
    torch = _require_gpu()
    v, f8, code, from_numpy, device = _as_device_inputs(torch, vis, flags)
    sel = None
    if select is not None:
        if not torch.is_tensor(select):
            select = torch.from_numpy(np.ascontiguousarray(select))
        sel = (select.to(device) != 0).view(torch.uint8)       # a device tensor stays there: no synchronisation
    return torch, v, f8, code, from_numpy, device, sel


def _bli_selected(nbl, sel):
    """Baselines that take part (the one host read of a selection; the accumulate alone does not need it)."""
    return nbl if sel is None else int(sel.sum().item())


def _bli_min_count(min_baseline_frac, nsel):
    import math
    return max(1, int(math.ceil(min_baseline_frac * nsel)))


def _bli_fraction(min_baseline_frac):
    frac = float(min_baseline_frac)
    if not 0.0 <= frac <= 1.0:                # also rejects NaN
        raise ValueError("min_baseline_frac must lie in [0, 1], got %r" % (min_baseline_frac,))
    return frac


def _acc_pair(torch, device, img, acc):
    """The accumulator of an integration over baselines: new (sum float64, count int32) tensors of shape `img` on the
    device -- zeros, or a copy of the pair `acc` to continue from (raises for a pair of another shape or dtype)."""
    if acc is None:
        return torch.zeros(img, dtype=torch.float64, device=device), torch.zeros(img, dtype=torch.int32, device=device)
    total, count = (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a for a in acc)
    if tuple(total.shape) != img or tuple(count.shape) != img:
        raise ValueError("acc must be a (sum, count) pair of shape %s" % (img,))
    if total.dtype != torch.float64 or count.dtype != torch.int32:
        raise TypeError("acc must be a (float64 sum, int32 count) pair")
    return total.to(device).clone().contiguous(), count.to(device).clone().contiguous()


def _bli_accumulate(torch, lib, device, v, f8, code, sel, acc):
    """(sum float64, count int32) of shape (corr, time, chan) on the device: new tensors, continued from `acc`."""
    nbl, img = int(v.shape[0]), tuple(int(s) for s in v.shape[1:])
    total, count = _acc_pair(torch, device, img, acc)
    if total.numel() > 0 and nbl > 0:
        _lib.check(lib.tri_baseline_accumulate(
            v.data_ptr(), code, f8.data_ptr(), sel.data_ptr() if sel is not None else None, nbl, total.numel(),
            total.data_ptr(), count.data_ptr(), torch.cuda.current_stream(device).cuda_stream))
    return total, count


def _bli_mean(torch, lib, device, total, count, min_count):
    amp = torch.empty(total.shape, dtype=torch.float32, device=device)
    flag = torch.empty(total.shape, dtype=torch.uint8, device=device)
    if total.numel() > 0:
        _lib.check(lib.tri_baseline_mean(total.data_ptr(), count.data_ptr(), total.numel(), min_count, amp.data_ptr(),
                                         flag.data_ptr(), torch.cuda.current_stream(device).cuda_stream))
    return amp, flag


def baseline_integral(vis, flags, select=None, acc=None):
    """Sum and count over baselines of the amplitudes of (bl, corr, time, chan)
    visibilities (complex64: ``|v|`` as the flagger takes it; float32:
    ``fabs``): for every (corr, time, chan) position and the baselines in
    ascending order, ``sum += float64(a)`` and ``count += 1`` over the samples
    whose baseline is selected (``select``, one entry per baseline, nonzero =
    takes part; None: all), whose flag is 0 and whose amplitude is not NaN.
    Returns ``(sum float64, count int32)`` of shape (corr, time, chan) --
    numpy arrays for numpy input, tensors on the device otherwise.  ``acc``:
    an earlier result to continue from (not modified; the result is a new
    pair): the baselines fed in several calls in ascending order give the bits
    of one call.  One thread owns a position and sums in memory order, so the
    result is reproducible bit for bit.  Inputs are not modified."""
    torch, v, f8, code, from_numpy, device, sel = _bli_inputs("baseline_integral", vis, flags, select)
    with torch.cuda.device(device):
        total, count = _bli_accumulate(torch, _lib.lib(), device, v, f8, code, sel, acc)
    return _like_input(from_numpy, total, count)


def baseline_mean_amplitude(vis, flags, select=None, min_baseline_frac=0.0):
    """Mean amplitude over baselines of (bl, corr, time, chan) visibilities:
    :func:`baseline_integral`'s ``float32(sum / count)`` per (corr, time, chan)
    position.  A position that fewer than ``max(1, ceil(min_baseline_frac *
    selected baselines))`` baselines count at is flagged, with amplitude 0.
    Returns ``(amp float32, flag bool)`` -- numpy arrays for numpy input,
    tensors on the device otherwise.  Inputs are not modified."""
    frac = _bli_fraction(min_baseline_frac)
    torch, v, f8, code, from_numpy, device, sel = _bli_inputs("baseline_mean_amplitude", vis, flags, select)
    nsel = _bli_selected(int(v.shape[0]), sel)
    lib = _lib.lib()
    with torch.cuda.device(device):
        total, count = _bli_accumulate(torch, lib, device, v, f8, code, sel, None)
        amp, flag = _bli_mean(torch, lib, device, total, count, _bli_min_count(frac, nsel))
    flag = flag.view(torch.bool)
    return _like_input(from_numpy, amp, flag)


def baseline_integrated_flagger(vis, flags, select=None, min_baseline_frac=0.25, **sum_threshold_kwargs):
    """SumThreshold on the baseline-integrated image (after AOFlagger's
    baseline integration): :func:`baseline_mean_amplitude` of the selected
    baselines gives one (corr, time, chan) float32 image whose noise falls as
    1 / sqrt(baselines); :func:`sum_threshold_flagger` (``sum_threshold_kwargs``)
    flags it as a (1, corr, time, chan) block; its detections are ORed into
    the flags of EVERY baseline, the unselected ones included:
    ``out[b] = (flags[b] != 0) | new``.  Finds RFI that is below the threshold
    of each baseline but present on all.  Returns a new array in the container
    / dtype of ``flags``; the inputs are not modified.  Parallelism is over the
    image alone: a short image with many baselines under-fills the device."""
    frac = _bli_fraction(min_baseline_frac)
    torch, v, f8, code, from_numpy, device, sel = _bli_inputs("baseline_integrated_flagger", vis, flags, select)
    nsel = _bli_selected(int(v.shape[0]), sel)
    lib = _lib.lib()
    nbl = int(v.shape[0])
    out = torch.empty(f8.shape, dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        if out.numel() > 0:
            total, count = _bli_accumulate(torch, lib, device, v, f8, code, sel, None)
            amp, flag = _bli_mean(torch, lib, device, total, count, _bli_min_count(frac, nsel))
            del total, count
            new = sum_threshold_flagger(amp[None], flag[None], **sum_threshold_kwargs)
            new8 = _flags_u8(torch, new, device)
            _lib.check(lib.tri_broadcast_or(f8.data_ptr(), new8.data_ptr(), out.data_ptr(), nbl, new8.numel(),
                                            torch.cuda.current_stream(device).cuda_stream))
    return _like_flags(torch, out, flags, from_numpy)


# ---------------------------------------------------------------------------
# Antenna integration: baseline integration with one image per antenna, and the
# flag excess of an antenna's baselines.  Python and C calls, not strategy tasks.
# ---------------------------------------------------------------------------
ANT_MAX_ANTENNAS = 65535


def _ant_ubl(ubl, nbl=None):
    ubl = np.asarray(ubl)
    if ubl.ndim != 2 or ubl.shape[1] != 3:
        raise ValueError("ubl must have shape (nbl, 3): (index, ant1, ant2) per baseline, got %s" % (ubl.shape,))
    if ubl.dtype.kind not in "iu":
        raise TypeError("ubl must hold integers, got %s" % ubl.dtype)
    if nbl is not None and ubl.shape[0] != nbl:
        raise ValueError("ubl must have one row per baseline (%d), got %d" % (nbl, ubl.shape[0]))
    return ubl


def antenna_baselines(ubl, nant=None, select=None, exclude_autos=True):
    """The per-antenna member lists of the antenna-integration calls, from
    ``ubl (nbl, 3)`` = (index, ant1, ant2) per baseline.  Baseline ``b`` is a
    member of antenna ``a`` if it is selected (``select``, one entry per
    baseline, nonzero = takes part; None: all), is not an auto-correlation
    where ``exclude_autos`` is set, and ``ant1[b] == a`` or ``ant2[b] == a``;
    an auto-correlation that takes part is a member of its antenna once.
    ``nant`` defaults to ``max(ant1, ant2) + 1``; a larger value is allowed and
    gives antennas without members.  Returns numpy int32 arrays ``(offsets
    (nant + 1), baselines, members (nant), ant1 (nbl), ant2 (nbl))``: the
    members of ``a`` are ``baselines[offsets[a]:offsets[a + 1]]`` in ascending
    order.  Pure host code; needs no device."""
    ubl = _ant_ubl(ubl)
    nbl = ubl.shape[0]
    a1, a2 = ubl[:, 1].astype(np.int64), ubl[:, 2].astype(np.int64)
    if nbl and (a1.min() < 0 or a2.min() < 0):
        raise ValueError("ubl holds a negative antenna number")
    need = int(max(a1.max(), a2.max())) + 1 if nbl else 0
    if nant is None:
        nant = need
    elif isinstance(nant, bool) or not isinstance(nant, (int, np.integer)):
        raise TypeError("nant must be an integer, got %r" % (nant,))
    elif nant < need:
        raise ValueError("nant = %d is below the largest antenna number + 1 = %d" % (nant, need))
    nant = int(nant)
    if nant > ANT_MAX_ANTENNAS:
        raise ValueError("nant = %d is above the %d antennas one call holds" % (nant, ANT_MAX_ANTENNAS))
    take = np.ones(nbl, bool)
    if select is not None:
        select = np.asarray(select.cpu() if hasattr(select, "cpu") else select)
        if select.shape != (nbl,):
            raise ValueError("select must have one entry per baseline (%d), got shape %s" % (nbl, select.shape))
        take = select != 0
    if exclude_autos:
        take = take & (a1 != a2)
    b = np.nonzero(take)[0]
    second = a2[b] != a1[b]                                    # an auto-correlation is a member once
    ants = np.concatenate([a1[b], a2[b][second]])
    bls = np.concatenate([b, b[second]])
    order = np.lexsort((bls, ants))                            # by antenna, ascending baseline within
    members = np.bincount(ants, minlength=nant).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(members)]).astype(np.int32)
    return offsets, bls[order].astype(np.int32), members, a1.astype(np.int32), a2.astype(np.int32)


def _ant_fraction(name, frac):
    value = float(frac)
    if not 0.0 <= value <= 1.0:               # also rejects NaN
        raise ValueError("%s must lie in [0, 1], got %r" % (name, frac))
    return value


def _ant_flags_inputs(flags, ubl, nant, select, exclude_autos):
    """Checks of the flags-only calls (all before any device work), then (torch, flags uint8 on the device, from_numpy,
    device, the host lists of antenna_baselines)."""
    shape = tuple(flags.shape)
    if len(shape) != 4:
        raise ValueError("flags must be 4-D (bl, corr, time, chan), got shape %s" % (shape,))
    lists = antenna_baselines(_ant_ubl(ubl, shape[0]), nant, select, exclude_autos)
    torch = _require_gpu()
    device = flags.device if (torch.is_tensor(flags) and flags.is_cuda) else \
        torch.device("cuda", torch.cuda.current_device())
    return torch, _flags_u8(torch, flags, device), isinstance(flags, np.ndarray), device, lists


def _ant_inputs(name, vis, flags, ubl, nant, select, exclude_autos):
    """Checks of the antenna-integration calls that read visibilities (all before any device work), then (torch, vis,
    flags uint8, dtype code, from_numpy, device, the host lists of antenna_baselines)."""
    shape = tuple(vis.shape)
    if len(shape) != 4:
        raise ValueError("vis must be 4-D (bl, corr, time, chan), got shape %s" % (shape,))
    if tuple(flags.shape) != shape:
        raise ValueError("vis and flags must have the same shape, got %s and %s" % (shape, tuple(flags.shape)))
    if str(vis.dtype).replace("torch.", "") not in ("complex64", "float32"):
        raise TypeError("tricolour_amd.%s: visibilities must be complex64 or float32 (got %s)" % (name, vis.dtype))
    lists = antenna_baselines(_ant_ubl(ubl, shape[0]), nant, select, exclude_autos)
    torch = _require_gpu()
    return (torch,) + _as_device_inputs(torch, vis, flags) + (lists,)


def _ant_dev(torch, device, a):
    """A host int32 list on the device; never empty, so that its address is one."""
    a = np.ascontiguousarray(a, np.int32)
    return torch.from_numpy(a if a.size else np.zeros(1, np.int32)).to(device)


def _ant_accumulate(torch, lib, device, v, f8, code, lists, acc):
    """(sum float64 or None, count int32) of shape (ant, corr, time, chan) on the device: new tensors, continued from
    `acc`.  v None: the flags-only count (acc: an earlier count)."""
    offsets, baselines, members = lists[:3]
    nbl, nant = int(f8.shape[0]), len(members)
    img = (nant,) + tuple(int(s) for s in f8.shape[1:])
    if v is None:
        total, count = None, torch.zeros(img, dtype=torch.int32, device=device)
    else:
        total, count = _acc_pair(torch, device, img, acc)
    if count.numel() > 0 and nbl > 0:
        off, bls = _ant_dev(torch, device, offsets), _ant_dev(torch, device, baselines)
        _lib.check(lib.tri_antenna_accumulate(
            None if v is None else v.data_ptr(), code, f8.data_ptr(), off.data_ptr(), bls.data_ptr(), nbl, nant,
            count.numel() // nant, None if total is None else total.data_ptr(), count.data_ptr(),
            torch.cuda.current_stream(device).cuda_stream))
    return total, count


def _ant_mean(torch, lib, device, total, count, members, frac):
    amp = torch.empty(total.shape, dtype=torch.float32, device=device)
    flag = torch.empty(total.shape, dtype=torch.uint8, device=device)
    if total.numel() > 0:
        min_count = np.maximum(1, np.ceil(frac * members.astype(np.float64))).astype(np.int32)
        mc = _ant_dev(torch, device, min_count)
        _lib.check(lib.tri_antenna_mean(total.data_ptr(), count.data_ptr(), mc.data_ptr(), len(members),
                                        total.numel() // len(members), amp.data_ptr(), flag.data_ptr(),
                                        torch.cuda.current_stream(device).cuda_stream))
    return amp, flag


def _ant_broadcast(torch, lib, device, f8, det8, ant1, ant2):
    out = torch.empty(f8.shape, dtype=torch.uint8, device=device)
    if out.numel() > 0:
        nbl, nant = int(f8.shape[0]), int(det8.shape[0])
        a1, a2 = _ant_dev(torch, device, ant1), _ant_dev(torch, device, ant2)
        _lib.check(lib.tri_antenna_broadcast_or(f8.data_ptr(), det8.data_ptr() if det8.numel() else None, a1.data_ptr(),
                                                a2.data_ptr(), out.data_ptr(), nbl, nant, out.numel() // nbl,
                                                torch.cuda.current_stream(device).cuda_stream))
    return out


def antenna_integral(vis, flags, ubl, nant=None, select=None, exclude_autos=True, acc=None):
    """Sum and count per antenna of the amplitudes of (bl, corr, time, chan)
    visibilities: :func:`baseline_integral` over the members of each antenna
    (:func:`antenna_baselines`) in ascending baseline order.  Returns ``(sum
    float64, count int32)`` of shape (ant, corr, time, chan) -- numpy arrays
    for numpy input, tensors on the device otherwise.  ``acc``: an earlier
    result to continue from (not modified; the result is a new pair): baseline
    chunks fed in ascending order, each call with its chunk's own ``ubl`` and
    the scan's ``nant``, give the bits of one call.  One thread owns a position
    of an antenna and sums in list order, so the result is reproducible bit
    for bit.  Every sample is read once per antenna it belongs to.  Inputs are
    not modified."""
    torch, v, f8, code, from_numpy, device, lists = _ant_inputs("antenna_integral", vis, flags, ubl, nant, select,
                                                                exclude_autos)
    with torch.cuda.device(device):
        total, count = _ant_accumulate(torch, _lib.lib(), device, v, f8, code, lists, acc)
    return _like_input(from_numpy, total, count)


def antenna_mean_amplitude(vis, flags, ubl, nant=None, select=None, exclude_autos=True, min_baseline_frac=0.0):
    """Mean amplitude per antenna: :func:`antenna_integral`'s ``float32(sum /
    count)`` per (ant, corr, time, chan) position.  A position that fewer than
    ``max(1, ceil(min_baseline_frac * members[ant]))`` baselines count at is
    flagged, with amplitude 0; an antenna without members is flagged
    throughout.  Returns ``(amp float32, flag bool)`` -- numpy arrays for numpy
    input, tensors on the device otherwise.  Inputs are not modified."""
    frac = _ant_fraction("min_baseline_frac", min_baseline_frac)
    torch, v, f8, code, from_numpy, device, lists = _ant_inputs("antenna_mean_amplitude", vis, flags, ubl, nant, select,
                                                                exclude_autos)
    lib = _lib.lib()
    with torch.cuda.device(device):
        total, count = _ant_accumulate(torch, lib, device, v, f8, code, lists, None)
        amp, flag = _ant_mean(torch, lib, device, total, count, lists[2], frac)
    return _like_input(from_numpy, amp, flag.view(torch.bool))


def antenna_integrated_flagger(vis, flags, ubl, nant=None, select=None, exclude_autos=True, min_baseline_frac=0.25,
                               **sum_threshold_kwargs):
    """SumThreshold on the antenna-integrated images: :func:`antenna_mean_amplitude`
    gives one (corr, time, chan) float32 image per antenna, whose noise falls
    as 1 / sqrt(members); :func:`sum_threshold_flagger` (``sum_threshold_kwargs``)
    flags them as an (ant, corr, time, chan) block; the detections of its two
    antennas are ORed into the flags of EVERY baseline, member of anything or
    not: ``out[b] = (flags[b] != 0) | det[ant1[b]] | det[ant2[b]]``.  Finds a
    fault that sits on the baselines of one antenna, too faint for each
    baseline alone and diluted over all baselines together.  Returns a new
    array in the container / dtype of ``flags``; the inputs are not modified.
    A Python call, not a strategy task."""
    frac = _ant_fraction("min_baseline_frac", min_baseline_frac)
    torch, v, f8, code, from_numpy, device, lists = _ant_inputs("antenna_integrated_flagger", vis, flags, ubl, nant,
                                                                select, exclude_autos)
    lib = _lib.lib()
    out = torch.empty(f8.shape, dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        if out.numel() > 0:
            total, count = _ant_accumulate(torch, lib, device, v, f8, code, lists, None)
            amp, flag = _ant_mean(torch, lib, device, total, count, lists[2], frac)
            del total, count
            det = sum_threshold_flagger(amp, flag, **sum_threshold_kwargs)
            out = _ant_broadcast(torch, lib, device, f8, _flags_u8(torch, det, device), lists[3], lists[4])
    return _like_flags(torch, out, flags, from_numpy)


def antenna_flagged_counts(flags, ubl, nant=None, select=None, exclude_autos=True):
    """How many of each antenna's member baselines (:func:`antenna_baselines`)
    are flagged at every (corr, time, chan) position.  No visibilities are
    read.  Returns ``(flagged int32 (ant, corr, time, chan), members int32
    (ant))`` -- numpy arrays for numpy input, tensors on the device otherwise."""
    torch, f8, from_numpy, device, lists = _ant_flags_inputs(flags, ubl, nant, select, exclude_autos)
    with torch.cuda.device(device):
        _, count = _ant_accumulate(torch, _lib.lib(), device, None, f8, 0, lists, None)
        members = torch.from_numpy(lists[2]).to(device)
        flagged = members.view(-1, 1, 1, 1) - count
    return _like_input(from_numpy, flagged, members)


def extend_flags_by_antenna(flags, ubl, nant=None, select=None, exclude_autos=True, min_flagged_frac=0.6):
    """Extends the flags of an antenna whose baselines are mostly flagged (after
    CASA's ``antint`` mode): where more than ``floor(min_flagged_frac *
    members[ant])`` of an antenna's member baselines are flagged at a (corr,
    time, chan) position, the position is flagged on EVERY baseline of that
    antenna: ``out[b] = (flags[b] != 0) | det[ant1[b]] | det[ant2[b]]``.
    ``min_flagged_frac`` lies in [0, 1]; 1.0 never adds a flag.  Flags only: no
    visibilities are read.  Returns a new array in the container / dtype of
    ``flags``; the input is not modified.  A Python call, not a strategy task."""
    frac = _ant_fraction("min_flagged_frac", min_flagged_frac)
    torch, f8, from_numpy, device, lists = _ant_flags_inputs(flags, ubl, nant, select, exclude_autos)
    lib = _lib.lib()
    members = lists[2]
    out = torch.empty(f8.shape, dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        if out.numel() > 0:
            _, count = _ant_accumulate(torch, lib, device, None, f8, 0, lists, None)
            max_flagged = np.floor(frac * members.astype(np.float64)).astype(np.int32)
            det = torch.empty(count.shape, dtype=torch.uint8, device=device)
            mem, mf = _ant_dev(torch, device, members), _ant_dev(torch, device, max_flagged)
            _lib.check(lib.tri_antenna_flag_excess(count.data_ptr(), mem.data_ptr(), mf.data_ptr(), len(members),
                                                   count.numel() // len(members), det.data_ptr(),
                                                   torch.cuda.current_stream(device).cuda_stream))
            out = _ant_broadcast(torch, lib, device, f8, det, lists[3], lists[4])
    return _like_flags(torch, out, flags, from_numpy)


def antenna_broadcast_or(flags, det, ubl, nant=None):
    """``out[b] = (flags[b] != 0) | (det[ant1[b]] != 0) | (det[ant2[b]] != 0)``
    for (bl, corr, time, chan) flags and per-antenna detections ``det`` of
    shape (ant, corr, time, chan); ``nant``, if given, is ``det.shape[0]``.  An
    antenna number of ``ubl`` outside ``[0, nant)`` contributes nothing.
    Returns a new array in the container / dtype of ``flags``; the inputs are
    not modified."""
    shape, dshape = tuple(flags.shape), tuple(det.shape)
    if len(shape) != 4:
        raise ValueError("flags must be 4-D (bl, corr, time, chan), got shape %s" % (shape,))
    if len(dshape) != 4 or dshape[1:] != shape[1:]:
        raise ValueError("det must have shape (ant,) + %s, got %s" % (shape[1:], dshape))
    if nant is not None and int(nant) != dshape[0]:
        raise ValueError("nant = %r is not the number of det images (%d)" % (nant, dshape[0]))
    if dshape[0] > ANT_MAX_ANTENNAS:
        raise ValueError("nant = %d is above the %d antennas one call holds" % (dshape[0], ANT_MAX_ANTENNAS))
    ubl = _ant_ubl(ubl, shape[0])
    # (clipped into int32: a number beyond it stays outside every antenna range)
    a1, a2 = (np.clip(ubl[:, k].astype(np.int64), -1, np.iinfo(np.int32).max).astype(np.int32) for k in (1, 2))
    torch = _require_gpu()
    device = flags.device if (torch.is_tensor(flags) and flags.is_cuda) else \
        torch.device("cuda", torch.cuda.current_device())
    f8, det8 = _flags_u8(torch, flags, device), _flags_u8(torch, det, device)
    with torch.cuda.device(device):
        out = _ant_broadcast(torch, _lib.lib(), device, f8, det8, a1, a2)
    return _like_flags(torch, out, flags, isinstance(flags, np.ndarray))


INS_MAX_SHAPES = 32


def _ins_number(name, v, lo, what):
    try:
        ok = isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and float(v) > lo   # also rejects NaN
    except (TypeError, ValueError):
        ok = False
    if not ok or float(v) == float("inf"):
        raise ValueError("%s must be %s, got %r" % (name, what, v))
    return float(v)


def _ins_index(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError("%s must be an integer, got %r" % (name, v))
    return int(v)


def check_incoherent_noise_kwargs(min_baseline_frac=0.25, nsigma=5.0, shapes=(), streak=True, narrow=True, rounds=3):
    """The argument checks of :func:`threshold_incoherent_noise_spectrum` that
    need no data (no device work): ``min_baseline_frac`` outside [0, 1], an
    ``nsigma`` that is not a finite number > 0, ``shapes`` entries that are not
    ``(lo, hi)`` or ``(lo, hi, nsigma)`` with integers ``0 <= lo < hi``, more
    than 32 shapes (the streak included), ``streak`` / ``narrow`` that are not
    booleans and ``rounds`` outside [1, 16] raise ``ValueError``.  Returns
    ``(frac, nsigma, [(lo, hi, nsigma), ...], streak, narrow, rounds)``."""
    try:
        frac = _bli_fraction(min_baseline_frac)
    except (TypeError, ValueError):
        raise ValueError("min_baseline_frac must lie in [0, 1], got %r" % (min_baseline_frac,))
    nsigma = _ins_number("nsigma", nsigma, 0.0, "a finite number > 0")
    for name, v in (("streak", streak), ("narrow", narrow)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError("%s must be True or False, got %r" % (name, v))
    if isinstance(rounds, bool) or not isinstance(rounds, (int, np.integer)) or not 1 <= int(rounds) <= 16:
        raise ValueError("rounds must be an integer in [1, 16], got %r" % (rounds,))
    try:
        entries = [tuple(s) for s in shapes]
    except TypeError:
        raise ValueError("shapes must be a sequence of (lo_chan, hi_chan) or (lo_chan, hi_chan, nsigma), got %r" % (shapes,))
    out = []
    for s in entries:
        if len(s) not in (2, 3):
            raise ValueError("a shape must be (lo_chan, hi_chan) or (lo_chan, hi_chan, nsigma), got %r" % (s,))
        lo, hi = _ins_index("shape lo_chan", s[0]), _ins_index("shape hi_chan", s[1])
        if not 0 <= lo < hi:
            raise ValueError("a shape needs 0 <= lo_chan < hi_chan, got %r" % (s,))
        out.append((lo, hi, _ins_number("shape nsigma", s[2], 0.0, "a finite number > 0") if len(s) == 3 else nsigma))
    if len(out) + (1 if streak else 0) > INS_MAX_SHAPES:
        raise ValueError("at most %d shapes (the streak included), got %d" % (INS_MAX_SHAPES, len(out) + (1 if streak else 0)))
    return frac, nsigma, out, bool(streak), bool(narrow), int(rounds)


def _ins_image_shape(shape):
    return (int(shape[1]), max(int(shape[2]) - 1, 0), int(shape[3]))


def _ins_accumulate(torch, lib, device, v, f8, code, sel, acc):
    """(sum float64, count int32) of shape (corr, time - 1, chan) on the device: new tensors, continued from `acc`."""
    nbl, ncorr, ntime, nchan = (int(s) for s in v.shape)
    total, count = _acc_pair(torch, device, _ins_image_shape(v.shape), acc)
    if total.numel() > 0 and nbl > 0:
        _lib.check(lib.tri_ins_accumulate(
            v.data_ptr(), code, f8.data_ptr(), sel.data_ptr() if sel is not None else None, nbl, ncorr, ntime, nchan,
            total.data_ptr(), count.data_ptr(), torch.cuda.current_stream(device).cuda_stream))
    return total, count


def _ins_check_acc(acc, img):
    if acc is None:
        return
    try:
        total, count = acc
    except (TypeError, ValueError):
        raise ValueError("acc must be a (sum, count) pair of shape %s" % (img,))
    if tuple(total.shape) != img or tuple(count.shape) != img:
        raise ValueError("acc must be a (sum, count) pair of shape %s" % (img,))
    if str(total.dtype).replace("torch.", "") != "float64" or str(count.dtype).replace("torch.", "") != "int32":
        raise TypeError("acc must be a (float64 sum, int32 count) pair")


def incoherent_noise_spectrum(vis, flags, select=None, acc=None):
    """Sum and count over baselines of the amplitudes of the time differences
    of (bl, corr, time, chan) visibilities (float32 input: amplitudes, ``im =
    0``): for every pair of rows ``(t, t + 1)`` and the baselines in ascending
    order, ``sum += float64(|v[t + 1] - v[t]|)`` (the difference in float32,
    its amplitude as the flagger takes it) and ``count += 1`` over the pairs
    whose baseline is selected (``select``, one entry per baseline, nonzero =
    takes part; None: all), whose two flags are 0 and whose amplitude is not
    NaN.  Sky and fringe vary slowly and cancel in the difference; noise and
    whatever changed between two dumps remain.  Returns ``(sum float64, count
    int32)`` of shape (corr, time - 1, chan) -- numpy arrays for numpy input,
    tensors on the device otherwise.  ``acc``: an earlier result to continue
    from (not modified; the result is a new pair): the baselines fed in
    several calls in ascending order give the bits of one call.  One thread
    owns a position and sums in memory order, so the result is reproducible
    bit for bit.  Definition: ``include/tricolour_amd.h``.  Inputs are not
    modified."""
    if len(tuple(vis.shape)) == 4:
        _ins_check_acc(acc, _ins_image_shape(vis.shape))
    torch, v, f8, code, from_numpy, device, sel = _bli_inputs("incoherent_noise_spectrum", vis, flags, select)
    with torch.cuda.device(device):
        total, count = _ins_accumulate(torch, _lib.lib(), device, v, f8, code, sel, acc)
    return _like_input(from_numpy, total, count)


def _ins_workspace(torch, lib, device, ncorr, ntime, nchan):
    nbytes = lib.tri_ins_workspace_bytes(ncorr, ntime, nchan)
    if nbytes == 0:
        raise NotImplementedError("incoherent noise spectrum: an image of (%d, %d, %d) is too large" % (ncorr, ntime - 1, nchan))
    return _workspace(torch, device, nbytes)


def incoherent_noise_zscore(sum, count, min_count, mask=None):
    """One round's z-score image of an :func:`incoherent_noise_spectrum`
    result ``(sum, count)`` of shape (corr, time - 1, chan): the level of each
    (corr, chan) line -- the median over time of the mean amplitudes
    ``float32(sum / count)`` of the usable (``count >= min_count``), unmasked
    positions --, the fixed-point z-score ``q`` (int32, units of 2**-16) and
    which positions are valid.  ``mask``: earlier detections of the same shape
    (None: none).  Returns ``(level float32 (corr, chan), q int32, valid
    bool)`` -- numpy arrays for numpy input, tensors on the device otherwise.
    Definition: ``include/tricolour_amd.h``.  Inputs are not modified."""
    img = tuple(sum.shape)
    if len(img) != 3:
        raise ValueError("sum must be 3-D (corr, time - 1, chan), got shape %s" % (img,))
    if tuple(count.shape) != img or (mask is not None and tuple(mask.shape) != img):
        raise ValueError("sum, count and mask must have the same shape, got %s, %s and %s"
                         % (img, tuple(count.shape), None if mask is None else tuple(mask.shape)))
    if str(sum.dtype).replace("torch.", "") != "float64" or str(count.dtype).replace("torch.", "") != "int32":
        raise TypeError("sum must be float64 and count int32, got %s and %s" % (sum.dtype, count.dtype))
    if isinstance(min_count, bool) or not isinstance(min_count, (int, np.integer)) or int(min_count) < 1:
        raise ValueError("min_count must be an integer >= 1, got %r" % (min_count,))
    torch = _require_gpu()
    from_numpy = not torch.is_tensor(sum)
    if from_numpy:
        device = torch.device("cuda", torch.cuda.current_device())
        s = torch.from_numpy(np.ascontiguousarray(sum)).to(device)
    else:
        if not sum.is_cuda:
            raise ValueError("tensors must live on the device")
        device = sum.device
        s = sum.contiguous()
    c = (torch.from_numpy(np.ascontiguousarray(count)) if not torch.is_tensor(count) else count).to(device).contiguous()
    if mask is None:
        m8 = torch.zeros(img, dtype=torch.uint8, device=device)
    else:
        m8 = _flags_u8(torch, torch.from_numpy(np.ascontiguousarray(mask)) if not torch.is_tensor(mask) else mask, device)
    ncorr, nd, nchan = (int(x) for x in img)
    level = torch.empty((ncorr, nchan), dtype=torch.float32, device=device)
    q = torch.empty(img, dtype=torch.int32, device=device)
    valid = torch.empty(img, dtype=torch.uint8, device=device)
    if s.numel() > 0:
        lib = _lib.lib()
        with torch.cuda.device(device):
            ws = _ins_workspace(torch, lib, device, ncorr, nd + 1, nchan)
            _lib.check(lib.tri_ins_zscore(s.data_ptr(), c.data_ptr(), m8.data_ptr(), ncorr, nd + 1, nchan, int(min_count),
                                          level.data_ptr(), q.data_ptr(), valid.data_ptr(), ws.data_ptr(), ws.numel(),
                                          torch.cuda.current_stream(device).cuda_stream))
    else:
        level.fill_(float("nan"))
    valid = valid.view(torch.bool)
    return _like_input(from_numpy, level, q, valid)


def _ins_match(torch, lib, device, total, count, min_count, shapes, nsigma_narrow, rounds):
    """The mask (corr, time - 1, chan) uint8 after `rounds` rounds; shapes: [(lo, hi, nsigma)]."""
    ncorr, nd, nchan = (int(x) for x in total.shape)
    mask = torch.empty(total.shape, dtype=torch.uint8, device=device)
    if total.numel() > 0:
        n = len(shapes)
        lo = (C.c_int64 * max(n, 1))(*[s[0] for s in shapes])
        hi = (C.c_int64 * max(n, 1))(*[s[1] for s in shapes])
        ns = (C.c_double * max(n, 1))(*[s[2] for s in shapes])
        ws = _ins_workspace(torch, lib, device, ncorr, nd + 1, nchan)
        _lib.check(lib.tri_ins_match(total.data_ptr(), count.data_ptr(), ncorr, nd + 1, nchan, min_count, lo, hi, ns, n,
                                     nsigma_narrow, rounds, mask.data_ptr(), ws.data_ptr(), ws.numel(),
                                     torch.cuda.current_stream(device).cuda_stream))
    return mask


def _ins_shapes(shapes, streak, nchan):
    """The step's shape list for `nchan` channels (raises ValueError for a shape beyond the band)."""
    for lo, hi, _ in shapes:
        if hi > nchan:
            raise ValueError("shape (%d, %d) does not lie within the %d channels" % (lo, hi, nchan))
    return list(shapes)


def threshold_incoherent_noise_spectrum(vis, flags, select=None, min_baseline_frac=0.25, nsigma=5.0, shapes=(),
                                        streak=True, narrow=True, rounds=3):
    """Flags (bl, corr, time, chan) windows on the sky-subtracted incoherent
    noise spectrum (after SSINS, Wilensky et al. 2019; the definition is this
    library's own, ``include/tricolour_amd.h``, and identity with SSINS is not
    claimed): :func:`incoherent_noise_spectrum` of the selected baselines
    gives the mean amplitude of the time differences per (corr, time pair,
    chan), whose noise falls as 1 / sqrt(baselines) and whose sigma is tied to
    its mean, so the z-score against the channel's median over time needs no
    background fit.  Per time pair, the matched sums of the z-scores over the
    channel ranges ``shapes`` -- entries ``(lo_chan, hi_chan)`` or ``(lo_chan,
    hi_chan, nsigma)``; ``streak`` appends the whole band ``(0, nchan)`` -- and,
    with ``narrow``, the largest single z-score are compared with ``nsigma``;
    the strongest candidate above it is flagged, and ``rounds`` rounds repeat
    this on what the earlier rounds left (a band and then a spike, or two
    bands, in one row).  A detection in the pair ``(t, t + 1)`` flags both
    times of its channels on EVERY baseline, the unselected ones included:
    ``out = (flags != 0) | mask[t - 1] | mask[t]``.  A position counts with at
    least ``max(1, ceil(min_baseline_frac * selected baselines))`` baselines.
    Finds faint RFI that is present on all baselines without fitting a
    background.  Returns a new array in the container / dtype of ``flags``; the
    inputs are not modified."""
    frac, nsigma, shapes, streak, narrow, rounds = check_incoherent_noise_kwargs(
        min_baseline_frac, nsigma, shapes, streak, narrow, rounds)
    if len(tuple(vis.shape)) == 4:
        nchan = int(vis.shape[3])
        shapes = _ins_shapes(shapes, streak, nchan)
        if streak and nchan > 0:
            shapes.append((0, nchan, nsigma))
    torch, v, f8, code, from_numpy, device, sel = _bli_inputs("threshold_incoherent_noise_spectrum", vis, flags, select)
    nbl, ncorr, ntime, nchan = (int(s) for s in v.shape)
    lib = _lib.lib()
    out = torch.empty(f8.shape, dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        if out.numel() > 0:
            nsel = _bli_selected(nbl, sel)
            total, count = _ins_accumulate(torch, lib, device, v, f8, code, sel, None)
            mask = _ins_match(torch, lib, device, total, count, _bli_min_count(frac, nsel), shapes,
                              nsigma if narrow else 0.0, rounds)
            del total, count
            if mask.numel() == 0:
                mask = torch.zeros(16, dtype=torch.uint8, device=device)     # ntime < 2: never read
            _lib.check(lib.tri_ins_apply(f8.data_ptr(), mask.data_ptr(), out.data_ptr(), nbl, ncorr, ntime, nchan,
                                         torch.cuda.current_stream(device).cuda_stream))
    return _like_flags(torch, out, flags, from_numpy)


def incoherent_noise_bands(bands_hz, chan_freq):
    """Channel ranges ``[(lo_chan, hi_chan), ...]`` of the frequency bands
    ``[[f_lo, f_hi], ...]``: a channel belongs to a band if its centre
    ``chan_freq[c]`` lies in ``[f_lo, f_hi]``; the range runs from the first to
    the last such channel, and a band without channels is dropped."""
    freq = np.asarray(chan_freq, np.float64).reshape(-1)
    out = []
    for f_lo, f_hi in bands_hz:
        inside = np.flatnonzero((freq >= float(f_lo)) & (freq <= float(f_hi)))
        if inside.size:
            out.append((int(inside[0]), int(inside[-1]) + 1))
    return out


def check_incoherent_noise_bands(bands_hz):
    """``bands_hz`` must be a sequence of ``[f_lo, f_hi]`` pairs of finite numbers with ``f_lo <= f_hi``."""
    try:
        pairs = [tuple(b) for b in bands_hz]
        ok = all(len(p) == 2 and not isinstance(p[0], bool) and not isinstance(p[1], bool)
                 and np.isfinite(float(p[0])) and np.isfinite(float(p[1])) and float(p[0]) <= float(p[1]) for p in pairs)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("bands_hz must be a list of [f_lo, f_hi] pairs of finite numbers with f_lo <= f_hi, got %r" % (bands_hz,))
    return [(float(a), float(b)) for a, b in pairs]
