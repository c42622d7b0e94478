"""Whole-scan flagging: the per-(field, ddid, scan) pipeline of the tricolour
application (``tricolour/apps/tricolour/app.py:370-486``) as one
device-resident call, plus the host pieces around it -- static masks
(``tricolour/mask.py:24-90``), strategy YAML and field / scan selection
(``app.py:327-368``).

:func:`flag_scan` runs residual, Stokes intensity, any-over-corr flags and
the window scatter in one kernel (``tri_pack_scan``), the window statistics,
the strategy chain of :mod:`tricolour_amd.strategies`, and the unpack with the
application's broadcast to the MS's correlations (``tri_unpack_scan``).  No
Measurement Set I/O: callers hand in columns already loaded.
"""
import logging
import numbers
import re
import threading
import time

import numpy as np

from tricolour_amd import packing
from tricolour_amd.stokes import STOKES_TYPES, stokes_corr_map
from tricolour_amd.strategies import STEPS, strategy_task

log = logging.getLogger(__name__)
_tls = threading.local()

VALID_TASKS = tuple(STEPS)         # the tasks of a strategy chain: one row each in strategies.STEPS
# steps that need every baseline of the scan at once: they cannot run per baseline chunk
WHOLE_SCAN_TASKS = tuple(t for t in STEPS if STEPS[t].whole_scan)


# ---------------------------------------------------------------------------
# static masks (mask.py:24-90)
# ---------------------------------------------------------------------------
def dilate_mask(mask_chans, mask_flags, dilate):
    """``mask_flags`` dilated by ``dilate`` channels, or by a width in
    ``Hz`` / ``kHz`` / ``MHz`` / ``GHz`` (``int(width / channel width) + 1``
    channels), as ``mask.dilate_mask`` does it with scipy's
    ``binary_dilation`` by ``[1, 1, 1]``: ``n`` iterations OR a +-n box with
    nothing beyond the band ends; ``n < 1`` repeats until nothing changes,
    i.e. the whole band if any channel is masked."""
    try:
        dilate_width = int(dilate)
    except ValueError:
        value, units = re.match(r"([\d.]+)([a-zA-Z]+)", dilate, re.I).groups()
        scale = {"GHz": 1e9, "MHz": 1e6, "kHz": 1e3, "Hz": 1.0}
        if units not in scale:
            raise ValueError('Unrecognised units for --dilate value::  %s' % units)
        value = float(value) * scale[units]
        chan_width = mask_chans[1] - mask_chans[0]
        dilate_width = int(value / chan_width) + 1
    flags = np.asarray(mask_flags, bool)
    if dilate_width < 1:
        return np.full(flags.shape, bool(flags.any()))
    n = min(dilate_width, flags.size)
    counts = np.concatenate([[0], np.cumsum(np.concatenate([np.zeros(n, np.int64), flags,
                                                            np.zeros(n, np.int64)]))])
    return (counts[2 * n + 1:] - counts[:-(2 * n + 1)]) > 0


def load_mask(filename, dilate):
    """Masked channel frequencies of a ``.staticmask`` file: a structured
    ``.npy`` array of dtype ``(bool, float64)`` whose row 0 holds the mask and
    row 1 the channel frequencies (mask.py:61-90).  Returns the ``(n, 1)``
    frequencies of the masked (after ``dilate``, if given) channels."""
    mask = np.load(filename)
    if mask.dtype[0] != bool or mask.dtype[1] != np.float64:
        raise ValueError("Mask %s is not a valid static mask "
                         "with labelled channel axis "
                         "[dtype == (bool, float64)]" % filename)
    mask_chans = mask["chans"][1]
    mask_flags = mask["mask"][0]
    if dilate:
        mask_flags = dilate_mask(mask_chans, mask_flags, dilate)
    masked_channels = mask_chans[np.argwhere(mask_flags)]
    log.info("Loaded mask {0:s} {1:s} with {2:.2f}% "
             "flagged bandwidth between {3:.3f} "
             "and {4:.3f} GHz".format(str(filename), "(dilated)" if dilate else "(non-dilated)",
                                      100.0 * masked_channels.size / mask_chans.size,
                                      np.min(mask_chans) / 1.0e9, np.max(mask_chans) / 1.0e9))
    return masked_channels


# ---------------------------------------------------------------------------
# configuration and selection
# ---------------------------------------------------------------------------
def load_strategies(path):
    """The ``strategies:`` list of a tricolour configuration YAML
    (``conf/default.yaml`` layout)."""
    import yaml
    with open(path) as fh:
        doc = yaml.safe_load(fh)
    if not isinstance(doc, dict) or not isinstance(doc.get("strategies"), list):
        raise ValueError("%s has no 'strategies' list" % path)
    return doc["strategies"]


def check_strategies(strategies):
    """Raises, before any work is done, the reference's errors for a strategy
    without a task or with an unknown one (strat_executor.py:33-36, 82-83), and
    the ``ValueError`` of each step's own pre-flight rules: its ``check`` in
    ``strategies.STEPS``, told whether a ``mark_missing`` step came before it."""
    marked = False
    for strategy in strategies:
        step = STEPS[strategy_task(strategy)]
        if step.check is not None:
            step.check(dict(strategy.get('kwargs') or {}), marked)
        marked = marked or step.marks


def _check_whole_scan_tasks(strategies, baseline_chunks):
    """A step that needs every baseline before it can flag any cannot run per baseline chunk."""
    if baseline_chunks is None:
        return
    for strategy in strategies:
        if strategy['task'] in WHOLE_SCAN_TASKS:
            raise ValueError("task '%s' needs every baseline of the scan at once and cannot run with baseline_chunks "
                             "set: flag the scan whole (baseline_chunks=None)" % strategy['task'])


def select_scans(scan_numbers, available):
    """Scans to flag (app.py:327-329): those of ``scan_numbers`` that exist,
    all of ``available`` when ``scan_numbers`` is None."""
    return list(set(available).intersection(scan_numbers if scan_numbers is not None else available))


def select_fields(field_names, fieldnames, ms_name=""):
    """``{field id: field name}`` to flag (app.py:335-368).  ``field_names``:
    user entries, each a name, a field index or a comma list of them;
    empty / None selects every field of ``fieldnames`` (the FIELD table's
    names).  Unknown names raise ``ValueError``."""
    fieldnames = list(fieldnames)
    if not field_names:
        return {i: fn for i, fn in enumerate(fieldnames)}
    flatten_field_names = []
    for f in field_names:
        flatten_field_names += [x.strip() for x in str(f).split(",")]
    for f in flatten_field_names:
        if re.match(r"^\d+$", f) and int(f) < len(fieldnames):
            flatten_field_names.append(fieldnames[int(f)])
    flatten_field_names = list(set(filter(lambda x: not re.match(r"^\d+$", x), flatten_field_names)))
    log.info("Only considering fields '{0:s}' for flagging per user "
             "selection criterion.".format(", ".join(flatten_field_names)))
    if not set(flatten_field_names) <= set(fieldnames):
        raise ValueError("One or more fields cannot be "
                         "found in dataset '{0:s}' "
                         "You specified {1:s}, but "
                         "only {2:s} are available".format(ms_name, ",".join(flatten_field_names),
                                                           ",".join(fieldnames)))
    return {fieldnames.index(fn): fn for fn in flatten_field_names}


# ---------------------------------------------------------------------------
# one scan
# ---------------------------------------------------------------------------
def _host(a, dtype=None):
    import torch
    if torch.is_tensor(a):
        a = a.cpu().numpy()
    a = np.asarray(a)
    return a.astype(dtype) if dtype is not None else a


def _stokes_terms(flagging_strategy, corr_type):
    if flagging_strategy == "standard":
        return ()
    if corr_type is None:
        raise ValueError("flagging strategy '%s' needs corr_type (the CORR_TYPE of the "
                         "polarisation table)" % flagging_strategy)
    codes = [STOKES_TYPES[c] if isinstance(c, str) else int(c) for c in _host(corr_type).tolist()]
    stokes_map = stokes_corr_map(codes)
    terms = tuple(v for k, v in stokes_map.items() if flagging_strategy == "total_power" or k != "I")
    if not terms:
        raise ValueError("correlations %s form no Stokes parameter for flagging strategy '%s'"
                         % (codes, flagging_strategy))
    return terms


def _check_baseline_chunks(baseline_chunks):
    if baseline_chunks is None:
        return None
    if isinstance(baseline_chunks, (bool, np.bool_)) or not isinstance(baseline_chunks, numbers.Integral):
        raise ValueError("baseline_chunks must be None or an integer >= 1, got %r" % (baseline_chunks,))
    if int(baseline_chunks) < 1:
        raise ValueError("baseline_chunks must be None or an integer >= 1, got %d" % int(baseline_chunks))
    return int(baseline_chunks)


def flag_scan(data, flags, antenna1, antenna2, time, chan_freq, chan_width, strategies, *, model=None,
              flagging_strategy="standard", corr_type=None, ignore_flags=False, antenna_positions=None,
              masked_channels=(), antenna_names=None, scan_no=0, field_name="", ddid=0, baseline_chunks=None,
              quality=None):
    """Flags one (field, ddid, scan) dataset as the tricolour application does
    (app.py:370-486).

    ``data`` / ``model`` / ``flags``: (row, chan, corr) columns (numpy or ROCm
    tensors); ``antenna1`` / ``antenna2`` / ``time``: per-row columns;
    ``chan_freq`` / ``chan_width``: the spectral window's channels;
    ``strategies``: the YAML's list of strategy dicts; ``flagging_strategy``:
    ``standard``, ``polarisation`` or ``total_power`` (the last two need
    ``corr_type``, casacore codes or names in dataset order);
    ``masked_channels``: a list of :func:`load_mask` results.

    Returns ``(row_flags, original_stats, final_stats)``: (row, chan, corr)
    bool flags, every correlation of a visibility flagged if any window
    correlation is (a numpy array for numpy ``data``, a device tensor
    otherwise), and the :class:`~tricolour_amd.window_statistics.WindowStatistics`
    of the packed flags before and after the strategies.

    ``baseline_chunks``: None holds the whole scan on the device at once; an
    integer N >= 1 streams it through the device in chunks of N consecutive
    baselines (:func:`tricolour_amd.packing.scan_chunks`), with the same
    flags and tallies.  Then only one chunk's rows, windows and row flags
    (and the next chunk's rows, in flight) are held on the device besides
    the caller's own device tensors, and host ``data`` (numpy or a CPU
    tensor) gives a numpy result.

    ``quality``: None, or a :class:`tricolour_amd.quality.ScanQuality` that is
    filled in place with the quality statistics of the packed windows (in the
    Stokes modes the residual or Stokes windows the strategies see) under the
    flags before and after the chain -- the same bits whole and streamed.
    ``ScanQuality(histograms=AmplitudeBins(...))`` takes the amplitude
    histograms of the kept and the flagged samples of the same windows as well
    (``original_histograms``, ``final_histograms``)."""
    import torch
    from tricolour_amd.strategies import apply_strategies
    from tricolour_amd.window_statistics import window_stats_block

    baseline_chunks = _check_baseline_chunks(baseline_chunks)
    _check_quality(quality)
    if flagging_strategy not in packing.SCAN_MODES:
        raise ValueError("Invalid flagging strategy '%s'" % flagging_strategy)
    strategies = list(strategies)
    check_strategies(strategies)
    _check_whole_scan_tasks(strategies, baseline_chunks)
    if len(tuple(data.shape)) != 3:
        raise ValueError("data must have shape (row, chan, corr), got %s" % (tuple(data.shape),))
    nrow, nchan, ncorr = (int(s) for s in data.shape)
    if not ignore_flags and flags is None:
        raise ValueError("flags are required unless ignore_flags is set")
    if flags is not None and tuple(flags.shape) != (nrow, nchan, ncorr):
        raise ValueError("flags shape %s != data shape %s" % (tuple(flags.shape), (nrow, nchan, ncorr)))
    if model is not None and tuple(model.shape) != (nrow, nchan, ncorr):
        raise ValueError("model shape %s != data shape %s" % (tuple(model.shape), (nrow, nchan, ncorr)))
    a1 = _host(antenna1, np.int32)
    a2 = _host(antenna2, np.int32)
    tm = _host(time)
    if not (a1.shape == a2.shape == tm.shape == (nrow,)):
        raise ValueError("antenna1 %s, antenna2 %s and time %s must have one entry per row (%d)"
                         % (a1.shape, a2.shape, tm.shape, nrow))
    chan_freq = _host(chan_freq, np.float64)
    chan_width = _host(chan_width, np.float64)
    if chan_freq.shape != (nchan,) or chan_width.shape != (nchan,):
        raise ValueError("chan_freq %s and chan_width %s must have one entry per channel (%d)"
                         % (chan_freq.shape, chan_width.shape, nchan))
    terms = _stokes_terms(flagging_strategy, corr_type)

    if ignore_flags:                                                           # app.py:403-410
        log.critical("Completely ignoring measurement set flags as per '-if' request. "
                     "Strategy WILL NOT or with original flags, even if specified!")
    if flagging_strategy == "total_power" and model is None:                  # :424-429
        log.critical("You requested to flag total quadrature power, but not on residuals. "
                     "This is not advisable and the flagger may mistake fringes of "
                     "off-axis sources for broadband RFI.")
    elif flagging_strategy == "standard" and model is None:                   # :434-439
        log.critical("You requested to flag per correlation, but not on residuals. "
                     "This is not advisable and the flagger may mistake fringes of off-axis sources "
                     "for broadband RFI.")

    from_numpy = not torch.is_tensor(data)
    ubl = packing.unique_baselines(a1, a2)                                     # :441-450
    utime, time_inv = np.unique(tm, return_inverse=True)
    time_inv = time_inv.reshape(-1).astype(np.int32)
    ntime = int(utime.shape[0])
    if antenna_names is None:
        nant = len(antenna_positions) if antenna_positions is not None else int(max(a1.max(initial=-1),
                                                                                    a2.max(initial=-1))) + 1
        antenna_names = [str(i) for i in range(nant)]
    antenna_names = [str(n) for n in _host(antenna_names).tolist()]

    ant_pos = None if antenna_positions is None else _host(antenna_positions)
    if baseline_chunks is not None and ubl.shape[0] > 0:
        return _flag_scan_streamed(
            data, None if ignore_flags else flags, model, a1, a2, time_inv, ntime, ubl, baseline_chunks,
            flagging_strategy, terms, strategies,
            dict(ant_pos=ant_pos, chan_freq=chan_freq, chan_width=chan_width, masked_channels=list(masked_channels)),
            (chan_freq, antenna_names, scan_no, field_name, ddid), _quality_begin(quality, ubl, chan_freq, utime))
    vis_w, flag_w = packing.pack_scan(time_inv, ubl, a1, a2, data, None if ignore_flags else flags, ntime,
                                      model=model, flagging_strategy=flagging_strategy, stokes_terms=terms)
    original = window_stats_block(flag_w, ubl, chan_freq, antenna_names, scan_no, field_name, ddid)
    quality = _quality_begin(quality, ubl, chan_freq, utime)
    _quality_add(quality, "original", vis_w, flag_w)
    flag_w = apply_strategies(strategies, flag_w, vis_w, ubl=ubl,
                              ant_pos=None if antenna_positions is None else _host(antenna_positions),
                              chan_freq=chan_freq, chan_width=chan_width, masked_channels=list(masked_channels))
    final = window_stats_block(flag_w, ubl, chan_freq, antenna_names, scan_no, field_name, ddid)
    _quality_add(quality, "final", vis_w, flag_w)
    row_flags = packing.unpack_scan(a1, a2, time_inv, ubl, flag_w, ncorr)     # :475-480
    if from_numpy:
        row_flags = row_flags.cpu().numpy()
    return row_flags, original, final


def _check_quality(quality):
    if quality is None:
        return
    from tricolour_amd.quality import ScanQuality
    if not isinstance(quality, ScanQuality):
        raise ValueError("quality must be None or a tricolour_amd.quality.ScanQuality, got %r" % (type(quality).__name__,))


def _quality_begin(quality, ubl, chan_freq, utime):
    """An emptied ``quality`` that knows its scan (None stays None)."""
    if quality is not None:
        quality.original = quality.final = None
        quality.original_histograms = quality.final_histograms = None
        quality.ubl, quality.chan_freq, quality.times = ubl, chan_freq, utime
    return quality


def _quality_add(quality, which, vis_w, flag_w):
    """The statistics of these windows, the scan's next baselines, onto ``quality.original`` or ``quality.final`` --
    and, if ``quality.histograms`` names bins, their amplitude histograms onto ``quality.<which>_histograms``."""
    if quality is not None:
        from tricolour_amd.quality import window_histograms, window_quality
        setattr(quality, which, window_quality(vis_w, flag_w, accumulate_into=getattr(quality, which)))
        if quality.histograms is not None:
            name = which + "_histograms"
            setattr(quality, name, window_histograms(vis_w, flag_w, quality.histograms, quality.freq_chunks,
                                                     accumulate_into=getattr(quality, name)))


def last_stream_stats():
    """Timings of this thread's latest streamed :func:`flag_scan` call (host
    inputs): ``upload_s`` / ``upload_bytes`` of the row uploads,
    ``upload_wait_s`` the part of it the flagging waited for (the rest ran
    under the previous chunk's work), ``d2h_s`` / ``d2h_bytes`` of the row
    flags returned, ``chunks``."""
    return dict(getattr(_tls, "stream_stats", {}))


def _host_rows(torch, a, dtype):
    """A host column as a CPU tensor without copying it (numpy, CPU or device tensor)."""
    if a is None:
        return None
    if torch.is_tensor(a):
        a = a.detach().cpu()
    else:
        a = torch.from_numpy(np.ascontiguousarray(a))
    if dtype == torch.bool and a.dtype not in (torch.bool, torch.uint8):
        a = a != 0
    return a.contiguous()


def _flag_scan_streamed(data, flags, model, a1, a2, time_inv, ntime, ubl, baseline_chunks, flagging_strategy, terms,
                        strategies, strategy_args, stats_args, quality=None):
    """:func:`flag_scan` one baseline chunk at a time.  For each chunk of
    :func:`~tricolour_amd.packing.scan_chunks`: its rows onto the device
    (device inputs: read in place through ``src_row``; host inputs: the
    chunk's runs of rows copied into a compact slab, on a side stream by a
    worker thread while the previous chunk is flagged), ``tri_fill_windows``
    + ``tri_pack_scan_rows``, the window statistics, the strategies on
    ``ubl[b0:b1]``, the statistics again and ``tri_unpack_scan_rows``.  The
    chunks' tallies are summed in baseline order, and so are the quality
    statistics if ``quality`` is given."""
    import contextlib
    from concurrent.futures import ThreadPoolExecutor

    from tricolour_amd import flagging
    from tricolour_amd.strategies import apply_strategies
    from tricolour_amd.window_statistics import window_stats_block

    torch = packing._torch_gpu()
    nrow, nchan, ncorr = (int(s) for s in data.shape)
    wcorr = ncorr if flagging_strategy == "standard" else 1
    on_device = torch.is_tensor(data) and data.is_cuda
    device = data.device if on_device else torch.device("cuda", torch.cuda.current_device())
    chunks = list(packing.scan_chunks(a1, a2, ubl, time_inv, ntime, baseline_chunks))
    link = flagging._H2D_TURN if flagging._LINK_TURNS else contextlib.nullcontext()
    times = dict(upload_s=0.0, upload_bytes=0, upload_wait_s=0.0, d2h_s=0.0, d2h_bytes=0, chunks=len(chunks))

    def idx(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(device)

    originals, finals = [], []
    with torch.cuda.device(device):
        main = torch.cuda.current_stream(device)
        if on_device:
            cols = [packing._dev(torch, data, torch.complex64),
                    None if model is None else packing._dev(torch, model, torch.complex64), None]
            if flags is not None:
                f = packing._dev(torch, flags)
                cols[2] = f.view(torch.uint8) if f.dtype == torch.bool else (f != 0).view(torch.uint8)
            result = torch.zeros((nrow, nchan, ncorr), dtype=torch.uint8, device=device)
        else:
            host = [_host_rows(torch, data, torch.complex64), _host_rows(torch, model, torch.complex64),
                    _host_rows(torch, flags, torch.bool)]
            slab_rows = max(c.rows.size for c in chunks)
            dtypes = (torch.complex64, torch.complex64, torch.bool)
            # two row slabs: chunk k + 1 is copied into one while chunk k is packed from the other
            slabs = [[None if h is None else torch.empty((slab_rows, nchan, ncorr), dtype=dt, device=device)
                      for h, dt in zip(host, dtypes)] for _ in range(2)]
            side = torch.cuda.Stream(device)
            result = np.zeros((nrow, nchan, ncorr), np.bool_)
            pool = ThreadPoolExecutor(max_workers=1)

            def upload(c, slot, after):
                # runs on the worker thread: the chunk's runs of rows into slot `slot`, once the main stream has
                # passed `after` (the last use of the slot and of any memory the slabs share)
                t0 = time.perf_counter()
                nbytes = 0
                with torch.cuda.device(device), torch.cuda.stream(side):
                    side.wait_event(after)
                    with link:
                        t1 = time.perf_counter()
                        j = 0
                        for r0, r1 in c.runs.tolist():
                            for h, dst in zip(host, slabs[slot]):
                                if h is not None:
                                    dst[j:j + r1 - r0].copy_(h[r0:r1], non_blocking=True)
                                    nbytes += dst[j:j + r1 - r0].nbytes
                            j += r1 - r0
                        side.synchronize()
                    done = torch.cuda.Event()
                    done.record(side)
                t2 = time.perf_counter()
                return done, t2 - t1, t2 - t0, nbytes

            def submit(k):
                after = torch.cuda.Event()
                after.record(main)
                return pool.submit(upload, chunks[k], k % 2, after)

        pending = None
        try:
            if not on_device:
                pending = submit(0)
            for k, c in enumerate(chunks):
                nbl_c, nr = c.b1 - c.b0, int(c.rows.size)
                whole_pack = c.pack.size == nr          # no duplicate cells in the chunk: pack every row
                if on_device:
                    src = idx(c.rows if whole_pack else c.rows[c.pack], np.int64)
                    data_c, model_c, flag_c = cols
                else:
                    t0 = time.perf_counter()
                    done, copy_s, _, nbytes = pending.result()
                    times["upload_wait_s"] += time.perf_counter() - t0
                    times["upload_s"] += copy_s
                    times["upload_bytes"] += nbytes
                    pending = None
                    main.wait_event(done)
                    src = None if whole_pack else idx(c.pack, np.int64)
                    data_c, model_c, flag_c = (None if s_ is None else s_[:nr] for s_ in slabs[k % 2])
                    if flag_c is not None:
                        flag_c = flag_c.view(torch.uint8)
                vis_w = torch.empty((nbl_c, wcorr, ntime, nchan), dtype=torch.complex64, device=device)
                flag_w = torch.empty((nbl_c, wcorr, ntime, nchan), dtype=torch.uint8, device=device)
                _lib_check_fill(torch, vis_w, flag_w)
                pb = c.bl if whole_pack else c.bl[c.pack]
                pt = c.time if whole_pack else c.time[c.pack]
                packing.pack_scan_rows(data_c, model_c, flag_c, src, idx(pb, np.int32), idx(pt, np.int32), nbl_c,
                                       ntime, vis_w, flag_w, flagging_strategy=flagging_strategy,
                                       stokes_terms=terms)
                if not on_device and k + 1 < len(chunks):
                    pending = submit(k + 1)               # under this chunk's statistics and strategies
                flag_w = flag_w.view(torch.bool)
                ubl_c = ubl[c.b0:c.b1]
                originals.append(window_stats_block(flag_w, ubl_c, *stats_args))
                _quality_add(quality, "original", vis_w, flag_w)
                flag_w = apply_strategies(strategies, flag_w, vis_w, ubl=ubl_c, **strategy_args)
                finals.append(window_stats_block(flag_w, ubl_c, *stats_args))
                _quality_add(quality, "final", vis_w, flag_w)
                del vis_w
                fw8 = flag_w.view(torch.uint8) if flag_w.dtype == torch.bool else (flag_w != 0).view(torch.uint8)
                ub, ut = idx(c.bl, np.int32), idx(c.time, np.int32)
                if on_device:
                    packing.unpack_scan_rows(fw8, idx(c.rows, np.int64), ub, ut, result)
                else:
                    out = torch.empty((nr, nchan, ncorr), dtype=torch.uint8, device=device)
                    packing.unpack_scan_rows(fw8, None, ub, ut, out)
                    _chunk_to_host(torch, flagging, link, main, out, c.rows, result, times)
        finally:
            if pending is not None:
                try:
                    pending.result()
                except Exception:
                    pass
            if not on_device:
                pool.shutdown()
                main.synchronize()
    flagging.release_workspace()
    _tls.stream_stats = times
    return (result.view(torch.bool) if on_device else result), _combine(originals), _combine(finals)


def _lib_check_fill(torch, vis_w, flag_w):
    from tricolour_amd import _lib
    stream = torch.cuda.current_stream(vis_w.device).cuda_stream
    _lib.check(_lib.lib().tri_fill_windows(vis_w.data_ptr(), flag_w.data_ptr(), vis_w.numel(), stream))


def _chunk_to_host(torch, flagging, link, main, out, rows, result, times):
    """A chunk's (rows, chan, corr) device flags into rows ``rows`` of the numpy ``result``: through this thread's
    pinned staging buffer (a copy into pageable pages runs at a fraction of the link rate), then a host scatter."""
    main.synchronize()
    t0 = time.perf_counter()
    stage = flagging._d2h_stage(torch, out.numel())
    with link:
        if stage is None:
            got = out.cpu().numpy()
        else:
            stage[:out.numel()].copy_(out.reshape(-1), non_blocking=True)
            main.synchronize()
            got = stage[:out.numel()].numpy().reshape(out.shape)
    times["d2h_s"] += time.perf_counter() - t0
    times["d2h_bytes"] += out.numel()
    result[rows] = got.view(np.bool_)


# ---------------------------------------------------------------------------
# every scan
# ---------------------------------------------------------------------------
def flag_scans(datasets, strategies, scan_numbers=None, field_names=None, *, fieldnames=None, ms_name="",
               flagging_strategy="standard", ignore_flags=False, antenna_positions=None, masked_channels=(),
               antenna_names=None, baseline_chunks=None, quality=None, histograms=None):
    """The dataset loop of the application (app.py:327-486) over datasets
    already loaded, one dict per (field, ddid, scan) with the keys
    ``DATA``, ``FLAG``, ``ANTENNA1``, ``ANTENNA2``, ``TIME``, ``FIELD_ID``,
    ``DATA_DESC_ID``, ``SCAN_NUMBER``, ``CHAN_FREQ``, ``CHAN_WIDTH``,
    ``CORR_TYPE`` (Stokes modes) and, to flag residuals, ``MODEL``.
    ``fieldnames``: names of the FIELD table (default ``"0"``, ``"1"``, ...).

    Returns ``(row_flags, summary)``: a list with the row flags of each
    dataset (None for datasets the field / scan selection skips) and the
    lines of ``summarise_stats`` over all flagged datasets (an empty list if
    none was flagged).  ``baseline_chunks``: as for :func:`flag_scan`.
    ``quality``: None, or a list to which one
    :class:`tricolour_amd.quality.ScanQuality` per flagged dataset is
    appended; ``histograms``: None, or the
    :class:`tricolour_amd.quality.AmplitudeBins` each of them is created with
    (it needs the ``quality`` list)."""
    from tricolour_amd.window_statistics import summarise_stats

    baseline_chunks = _check_baseline_chunks(baseline_chunks)
    datasets = list(datasets)
    strategies = list(strategies)
    check_strategies(strategies)
    _check_whole_scan_tasks(strategies, baseline_chunks)
    if quality is not None and not isinstance(quality, list):
        raise ValueError("quality must be None or a list, got %r" % (type(quality).__name__,))
    if histograms is not None:
        from tricolour_amd.quality import ScanQuality
        if quality is None:
            raise ValueError("histograms needs a quality list to append to")
        ScanQuality(histograms=histograms)              # raises ValueError for anything but bins
    if fieldnames is None:
        nfield = max([int(ds["FIELD_ID"]) for ds in datasets], default=-1) + 1
        fieldnames = [str(i) for i in range(nfield)]
    scans = select_scans(scan_numbers, [int(ds["SCAN_NUMBER"]) for ds in datasets])
    if scans != []:
        log.info("Only considering scans '{0:s}' as per user selection criterion"
                 .format(", ".join(map(str, map(int, scans)))))
    field_dict = select_fields(field_names, fieldnames, ms_name)

    out, original_stats, final_stats = [], [], []
    for ds in datasets:
        field_id, scan_no = int(ds["FIELD_ID"]), int(ds["SCAN_NUMBER"])
        if field_id not in field_dict or scan_no not in scans:
            out.append(None)
            continue
        log.info("Flagging field '{0:s}' scan {1:d}".format(field_dict[field_id], scan_no))
        one = None
        if quality is not None:
            from tricolour_amd.quality import ScanQuality
            one = ScanQuality(histograms=histograms)
        row_flags, original, final = flag_scan(
            ds["DATA"], ds.get("FLAG"), ds["ANTENNA1"], ds["ANTENNA2"], ds["TIME"], ds["CHAN_FREQ"],
            ds["CHAN_WIDTH"], strategies, model=ds.get("MODEL"), flagging_strategy=flagging_strategy,
            corr_type=ds.get("CORR_TYPE"), ignore_flags=ignore_flags, antenna_positions=antenna_positions,
            masked_channels=masked_channels, antenna_names=antenna_names, scan_no=scan_no,
            field_name=field_dict[field_id], ddid=int(ds["DATA_DESC_ID"]), baseline_chunks=baseline_chunks,
            quality=one)
        if one is not None:
            quality.append(one)
        out.append(row_flags)
        original_stats.append(original)
        final_stats.append(final)
    if not final_stats:
        return out, []
    return out, summarise_stats(_combine(final_stats), _combine(original_stats))


def _combine(stats):
    """combine_window_stats (window_statistics.py:143-168) of computed tallies."""
    total = stats[0].copy()
    for one in stats[1:]:
        total.update(one)
    return total
