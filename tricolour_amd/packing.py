"""Window packing on the device: MS row order (row, chan, corr) <-> windows
(bl, corr, time, chan).  Mirrors ``tricolour/packing.py`` for the in-HBM
("numpy") backend; the zarr-disk spill store is out of scope (windows live in
288 GB of HBM instead).

The reference matches every row against every baseline
(``_numba_pack_data``, packing.py:262-276, O(nbl * rows)); here the
``row -> (baseline, time)`` map is computed once on the host
(:func:`row_map`) and the scatter / gather run as HIP kernels.
"""
import numpy as np

from tricolour_amd import _lib

_WINDOW_SCHEMA = ("bl", "corr", "time", "chan")    # packing.py:15


def unique_baselines(ant1, ant2):
    """(nbl, 3) int32 rows ``(bl_index, ant1, ant2)`` in the reference's
    order: ascending 64-bit value of the (ant1, ant2) int32 pair viewed as one
    little-endian int64, i.e. sorted by (ant2, ant1) (packing.py:36-56,
    apps/tricolour/app.py:444-450)."""
    ant1 = np.ascontiguousarray(ant1)
    ant2 = np.ascontiguousarray(ant2)
    if not (ant1.dtype == np.int32 and ant2.dtype == np.int32):
        raise TypeError("antenna1 '%s' and antenna2 '%s' dtypes "
                        "must both be np.int32" % (ant1.dtype, ant2.dtype))
    bl = np.stack([ant1, ant2], axis=1).copy().view(np.int64).reshape(-1)
    u = np.unique(bl)
    pairs = u.view(np.int32).reshape(-1, 2)
    idx = np.arange(pairs.shape[0], dtype=np.int32)[:, None]
    return np.concatenate([idx, pairs], axis=1).astype(np.int32)


def row_map(ant1, ant2, ubl, time_inv, ntime=None):
    """Per-row window coordinates: ``row_bl[r]`` = position in ``ubl`` of the
    row's baseline (-1 if absent), ``row_time[r] = time_inv[r]``.  When
    several rows map to the same (baseline, time) cell the reference's serial
    loop lets the LAST row win (packing.py:262-276); earlier duplicates are
    masked out here so that the parallel scatter is deterministic and equal."""
    ant1 = np.asarray(ant1, np.int64)
    ant2 = np.asarray(ant2, np.int64)
    ubl = np.asarray(ubl)
    key = ubl[:, 1].astype(np.int64) | (ubl[:, 2].astype(np.int64) << 32)
    order = np.argsort(key, kind="stable")
    rkey = ant1 | (ant2 << 32)
    pos = np.searchsorted(key[order], rkey)
    pos_c = np.clip(pos, 0, max(len(key) - 1, 0))
    found = (len(key) > 0) & (pos < len(key))
    if len(key):
        found = found & (key[order][pos_c] == rkey)
    row_bl = np.where(found, order[pos_c] if len(key) else 0, -1).astype(np.int32)
    row_time = np.asarray(time_inv, np.int32).copy()
    if ntime is None:
        ntime = int(row_time.max()) + 1 if row_time.size else 0
    cell = row_bl.astype(np.int64) * max(int(ntime), 1) + row_time
    valid = row_bl >= 0
    # keep only the last row of each occupied cell
    rev = np.arange(len(cell))[::-1]
    _, first_in_rev = np.unique(cell[rev], return_index=True)
    keep = np.zeros(len(cell), bool)
    keep[rev[first_in_rev]] = True
    row_bl_pack = np.where(valid & keep, row_bl, -1).astype(np.int32)
    return row_bl, row_bl_pack, row_time


def _torch_gpu():
    import torch
    _lib.lib()
    if not torch.cuda.is_available():
        raise RuntimeError("tricolour_amd.packing needs a ROCm GPU; there is no CPU fallback")
    return torch


def _dev(torch, a, dtype=None):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a))
    a = a.cuda() if not a.is_cuda else a
    if dtype is not None and a.dtype != dtype:
        a = a.to(dtype)
    return a.contiguous()


def pack_data(time_inv, ubl, antenna1, antenna2, data, flags, ntime):
    """Device version of ``packing.pack_data`` (packing.py:306-366) for one
    dataset: returns ``(vis_windows, flag_windows)`` torch tensors of shape
    (bl, corr, time, chan); cells no row maps to hold NaN+NaNj / True
    (packing.py:97,117)."""
    torch = _torch_gpu()
    lib = _lib.lib()
    ubl = np.asarray(ubl)
    rows, nchan, ncorr = (int(s) for s in data.shape)
    if tuple(flags.shape) != tuple(data.shape):
        raise ValueError("vis_windows.shape != flag_windows.shape")   # packing.py:253
    nbl = int(ubl.shape[0])
    _, row_bl, row_time = row_map(np.asarray(antenna1), np.asarray(antenna2), ubl,
                                  np.asarray(time_inv), ntime)
    d = _dev(torch, data, torch.complex64)
    f = _dev(torch, flags)
    f8 = f.view(torch.uint8) if f.dtype == torch.bool else (f != 0).view(torch.uint8)
    rb, rt = _dev(torch, row_bl), _dev(torch, row_time)
    vis_w = torch.empty((nbl, ncorr, int(ntime), nchan), dtype=torch.complex64, device=d.device)
    flag_w = torch.empty((nbl, ncorr, int(ntime), nchan), dtype=torch.uint8, device=d.device)
    stream = torch.cuda.current_stream(d.device).cuda_stream
    _lib.check(lib.tri_fill_windows(vis_w.data_ptr(), flag_w.data_ptr(), vis_w.numel(), stream))
    _lib.check(lib.tri_pack_data(d.data_ptr(), f8.data_ptr(), rb.data_ptr(), rt.data_ptr(),
                                 rows, nchan, ncorr, nbl, int(ntime), vis_w.data_ptr(),
                                 flag_w.data_ptr(), stream))
    return vis_w, flag_w.view(torch.bool)


def unpack_data(antenna1, antenna2, time_inv, ubl, flag_windows, equalize_corr=False):
    """Device version of ``packing.unpack_data`` (packing.py:391-425): gathers
    flag windows back to (row, chan, corr); rows whose baseline is not in
    ``ubl`` stay 0.  ``equalize_corr=True`` additionally flags every
    correlation of a visibility if any is flagged (the step the application
    applies right after unpacking, apps/tricolour/app.py:479-480)."""
    torch = _torch_gpu()
    lib = _lib.lib()
    ubl = np.asarray(ubl)
    nbl, ncorr, ntime, nchan = (int(s) for s in flag_windows.shape)
    if nbl != int(ubl.shape[0]):
        raise ValueError("flag_windows and ubl disagree on the number of baselines")
    row_bl, _, row_time = row_map(np.asarray(antenna1), np.asarray(antenna2), ubl,
                                  np.asarray(time_inv), ntime)
    rows = len(row_bl)
    fw = _dev(torch, flag_windows)
    fw8 = fw.view(torch.uint8) if fw.dtype == torch.bool else (fw != 0).view(torch.uint8)
    rb, rt = _dev(torch, row_bl), _dev(torch, row_time)
    out = torch.empty((rows, nchan, ncorr), dtype=torch.uint8, device=fw.device)
    stream = torch.cuda.current_stream(fw.device).cuda_stream
    _lib.check(lib.tri_unpack_data(fw8.data_ptr(), rb.data_ptr(), rt.data_ptr(), rows, nchan,
                                   ncorr, nbl, ntime, out.data_ptr(), 1 if equalize_corr else 0, stream))
    return out.view(torch.bool)


SCAN_MODES = {"standard": 0, "polarisation": 1, "total_power": 2}


def pack_scan(time_inv, ubl, antenna1, antenna2, data, flags, ntime, model=None,
              flagging_strategy="standard", stokes_terms=()):
    """The input side of one scan (apps/tricolour/app.py:389-457) in one pass
    over the MS rows (``tri_pack_scan``): ``vis = data - model`` (``model``
    None: ``data``), the polarised intensity of ``stokes_terms`` (the
    ``(c1, c2, a, s1, s2)`` tuples of :func:`tricolour_amd.stokes.stokes_corr_map`)
    and any-over-corr flags in the ``polarisation`` / ``total_power`` modes,
    then the scatter of :func:`pack_data`.  ``flags`` None: all unflagged
    (``--ignore-flags``).  Returns ``(vis_windows, flag_windows)`` of shape
    (bl, wcorr, time, chan), wcorr = ncorr in ``standard`` mode and 1
    otherwise; data and model are taken as complex64, as :func:`pack_data`
    does."""
    from tricolour_amd.stokes import _term_tables
    if flagging_strategy not in SCAN_MODES:
        raise ValueError("Invalid flagging strategy '%s'" % flagging_strategy)
    mode = SCAN_MODES[flagging_strategy]
    if len(tuple(data.shape)) != 3:
        raise ValueError("data must have shape (row, chan, corr)")
    rows, nchan, ncorr = (int(s) for s in data.shape)
    if flags is not None and tuple(flags.shape) != tuple(data.shape):
        raise ValueError("flags shape %s != data shape %s" % (tuple(flags.shape), tuple(data.shape)))
    if model is not None and tuple(model.shape) != tuple(data.shape):
        raise ValueError("model shape %s != data shape %s" % (tuple(model.shape), tuple(data.shape)))
    if mode != 0 and len(tuple(stokes_terms)) == 0:
        raise ValueError("flagging strategy '%s' needs stokes terms" % flagging_strategy)
    torch = _torch_gpu()
    lib = _lib.lib()
    ubl = np.asarray(ubl)
    nbl = int(ubl.shape[0])
    ntime = int(ntime)
    _, row_bl, row_time = row_map(np.asarray(antenna1), np.asarray(antenna2), ubl,
                                  np.asarray(time_inv), ntime)
    d = _dev(torch, data, torch.complex64)
    m = None if model is None else _dev(torch, model, torch.complex64)
    f8 = None
    if flags is not None:
        f = _dev(torch, flags)
        f8 = f.view(torch.uint8) if f.dtype == torch.bool else (f != 0).view(torch.uint8)
    rb, rt = _dev(torch, row_bl), _dev(torch, row_time)
    wcorr = ncorr if mode == 0 else 1
    vis_w = torch.empty((nbl, wcorr, ntime, nchan), dtype=torch.complex64, device=d.device)
    flag_w = torch.empty((nbl, wcorr, ntime, nchan), dtype=torch.uint8, device=d.device)
    pidx, palpha, npol = _term_tables(stokes_terms if mode != 0 else ())
    stream = torch.cuda.current_stream(d.device).cuda_stream
    _lib.check(lib.tri_fill_windows(vis_w.data_ptr(), flag_w.data_ptr(), vis_w.numel(), stream))
    _lib.check(lib.tri_pack_scan(d.data_ptr(), None if m is None else m.data_ptr(),
                                 None if f8 is None else f8.data_ptr(), rb.data_ptr(), rt.data_ptr(),
                                 rows, nchan, ncorr, nbl, ntime, mode,
                                 pidx.ctypes.data, palpha.ctypes.data, npol,
                                 vis_w.data_ptr(), flag_w.data_ptr(), stream))
    return vis_w, flag_w.view(torch.bool)


def unpack_scan(antenna1, antenna2, time_inv, ubl, flag_windows, ncorr):
    """The MS flags of a scan (apps/tricolour/app.py:475-480) from its
    (bl, wcorr, time, chan) flag windows (``tri_unpack_scan``): any over the
    window correlations, broadcast to ``ncorr`` correlations, as a
    (row, chan, ncorr) bool tensor; rows whose baseline is not in ``ubl``
    stay 0.  ``wcorr`` must be 1 or ``ncorr``."""
    torch = _torch_gpu()
    lib = _lib.lib()
    ubl = np.asarray(ubl)
    nbl, wcorr, ntime, nchan = (int(s) for s in flag_windows.shape)
    ncorr = int(ncorr)
    if nbl != int(ubl.shape[0]):
        raise ValueError("flag_windows and ubl disagree on the number of baselines")
    if wcorr not in (1, ncorr):
        raise ValueError("flag windows have %d correlations: need 1 or %d" % (wcorr, ncorr))
    row_bl, _, row_time = row_map(np.asarray(antenna1), np.asarray(antenna2), ubl,
                                  np.asarray(time_inv), ntime)
    rows = len(row_bl)
    fw = _dev(torch, flag_windows)
    fw8 = fw.view(torch.uint8) if fw.dtype == torch.bool else (fw != 0).view(torch.uint8)
    rb, rt = _dev(torch, row_bl), _dev(torch, row_time)
    out = torch.empty((rows, nchan, ncorr), dtype=torch.uint8, device=fw.device)
    stream = torch.cuda.current_stream(fw.device).cuda_stream
    _lib.check(lib.tri_unpack_scan(fw8.data_ptr(), rb.data_ptr(), rt.data_ptr(), rows, nchan, wcorr,
                                   ncorr, nbl, ntime, out.data_ptr(), stream))
    return out.view(torch.bool)


class ScanChunk:
    """One baseline chunk ``[b0, b1)`` of a scan (:func:`scan_chunks`).

    ``rows``: every MS row of the chunk's baselines, ascending (int64), the
    unpack list; ``bl``: the rows' baseline within the chunk (``row_bl - b0``,
    int32); ``time``: their time index (int32); ``pack``: positions in
    ``rows`` of the rows :func:`row_map` keeps for packing (int64, ascending);
    ``runs``: ``(n, 2)`` int64 ``[start, stop)`` of the maximal runs of
    consecutive MS rows in ``rows``, in order."""
    __slots__ = ("b0", "b1", "rows", "bl", "time", "pack", "runs")

    def __init__(self, b0, b1, rows, bl, time, pack, runs):
        self.b0, self.b1, self.rows, self.bl, self.time, self.pack, self.runs = b0, b1, rows, bl, time, pack, runs

    @property
    def pack_rows(self):
        return self.rows[self.pack]


def scan_chunks(ant1, ant2, ubl, time_inv, ntime, baseline_chunks):
    """Splits a scan into chunks of ``baseline_chunks`` consecutive baselines
    of ``ubl`` and yields one :class:`ScanChunk` per chunk, in baseline order.
    Every row whose baseline is in ``ubl`` lies in exactly one chunk; when rows
    duplicate a (baseline, time) cell, the pack list keeps the last one, as
    :func:`row_map` does."""
    n = int(baseline_chunks)
    if n < 1:
        raise ValueError("baseline_chunks must be >= 1, got %d" % n)
    ubl = np.asarray(ubl)
    nbl = int(ubl.shape[0])
    row_bl, row_bl_pack, row_time = row_map(np.asarray(ant1), np.asarray(ant2), ubl, np.asarray(time_inv), ntime)
    mapped = np.nonzero(row_bl >= 0)[0]
    chunk = row_bl[mapped] // n
    order = mapped[np.argsort(chunk, kind="stable")]          # rows grouped by chunk, ascending within one
    bounds = np.searchsorted(np.sort(chunk, kind="stable"), np.arange(-(-nbl // n) + 1))
    for k in range(len(bounds) - 1):
        rows = order[bounds[k]:bounds[k + 1]].astype(np.int64)
        b0 = k * n
        cut = np.nonzero(np.diff(rows) != 1)[0] + 1
        starts = np.concatenate([[0], cut]).astype(np.int64)
        stops = np.concatenate([cut, [rows.size]]).astype(np.int64)
        runs = np.stack([rows[starts], rows[stops - 1] + 1], axis=1) if rows.size else np.zeros((0, 2), np.int64)
        yield ScanChunk(b0, min(b0 + n, nbl), rows, (row_bl[rows] - b0).astype(np.int32), row_time[rows],
                        np.nonzero(row_bl_pack[rows] >= 0)[0].astype(np.int64), runs)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _term_args(mode, stokes_terms):
    from tricolour_amd.stokes import _term_tables
    return _term_tables(stokes_terms if mode != 0 else ())


def pack_scan_rows(data, model, flags, src_row, row_bl, row_time, nbl, ntime, vis_windows, flag_windows,
                   flagging_strategy="standard", stokes_terms=()):
    """``tri_pack_scan_rows`` on device tensors: entry ``i`` of the lists
    packs row ``src_row[i]`` (None: row ``i``) of the (rows, chan, corr)
    ``data`` (complex64), ``model`` (complex64 or None) and ``flags`` (uint8
    or None) into cell ``(row_bl[i], row_time[i])`` of the (nbl, wcorr,
    ntime, chan) windows, on the current stream.  ``src_row``: int64,
    ``row_bl`` / ``row_time``: int32 device tensors."""
    import torch
    lib = _lib.lib()
    mode = SCAN_MODES[flagging_strategy]
    src_rows, nchan, ncorr = (int(s) for s in data.shape)
    for name, col in (("model", model), ("flags", flags)):
        if col is not None and tuple(col.shape) != tuple(data.shape):
            raise ValueError("%s shape %s != data shape %s" % (name, tuple(col.shape), tuple(data.shape)))
    if not (row_bl.numel() == row_time.numel() and (src_row is None or src_row.numel() == row_bl.numel())):
        raise ValueError("src_row, row_bl and row_time must have one entry per list entry")
    pidx, palpha, npol = _term_args(mode, stokes_terms)
    stream = torch.cuda.current_stream(data.device).cuda_stream
    _lib.check(lib.tri_pack_scan_rows(data.data_ptr(), _ptr(model), _ptr(flags), _ptr(src_row), src_rows,
                                      row_bl.data_ptr(), row_time.data_ptr(), int(row_bl.numel()), nchan, ncorr,
                                      int(nbl), int(ntime), mode, pidx.ctypes.data, palpha.ctypes.data, npol,
                                      vis_windows.data_ptr(), flag_windows.data_ptr(), stream))


def unpack_scan_rows(flag_windows, dst_row, row_bl, row_time, out):
    """``tri_unpack_scan_rows`` on device tensors: entry ``i`` writes row
    ``dst_row[i]`` (None: row ``i``) of the (rows, chan, ncorr) uint8 ``out``
    from cell ``(row_bl[i], row_time[i])`` of the (bl, wcorr, time, chan)
    ``flag_windows``, on the current stream; other rows keep their contents."""
    import torch
    lib = _lib.lib()
    nbl, wcorr, ntime, nchan = (int(s) for s in flag_windows.shape)
    out_rows, onchan, ncorr = (int(s) for s in out.shape)
    if onchan != nchan:
        raise ValueError("flag windows have %d channels, the output %d" % (nchan, onchan))
    if wcorr not in (1, ncorr):
        raise ValueError("flag windows have %d correlations: need 1 or %d" % (wcorr, ncorr))
    if not (row_bl.numel() == row_time.numel() and (dst_row is None or dst_row.numel() == row_bl.numel())):
        raise ValueError("dst_row, row_bl and row_time must have one entry per list entry")
    stream = torch.cuda.current_stream(out.device).cuda_stream
    _lib.check(lib.tri_unpack_scan_rows(flag_windows.data_ptr(), _ptr(dst_row), out_rows, row_bl.data_ptr(),
                                        row_time.data_ptr(), int(row_bl.numel()), nchan, wcorr, ncorr, nbl, ntime,
                                        out.data_ptr(), stream))
