#!/opt/conda/bin/python3.9
"""Generates G15 (whole-scan flagging) with the reference's own packing.py,
stokes.py, StrategyExecutor, window_statistics.py and mask.load_mask, driven
through the per-scan steps of apps/tricolour/app.py:370-486 written out below
(app.py itself needs dask-ms).  Run un-jitted under /opt/conda/bin/python3.9
(the interpreter with dask and scipy) with the refshim numba stand-in, a stub
zarr (only the zarr-disk backend uses it) and a stub tricolour.config (the
mask search paths).  Build-container only; just the .npz data travels.

    cd tests/golden && PYTHONDONTWRITEBYTECODE=1 /opt/conda/bin/python3.9 make_golden_scan.py
"""
import hashlib
import json
import os
import sys
import tempfile
import time
import types
import warnings

import numpy as np

warnings.filterwarnings("ignore")
if not hasattr(np, "exceptions"):
    np.exceptions = types.SimpleNamespace(RankWarning=np.RankWarning)
elif not hasattr(np.exceptions, "RankWarning"):
    np.exceptions.RankWarning = np.RankWarning

zarr = types.ModuleType("zarr")
zarr.Array = type("Array", (), {})
zarr.ThreadSynchronizer = lambda *a, **k: None
sys.modules["zarr"] = zarr

from refshim import load_reference_flagging  # noqa: E402

load_reference_flagging()
config = types.ModuleType("tricolour.config")
config.paths = []
sys.modules["tricolour.config"] = config

import dask  # noqa: E402
import dask.array as da  # noqa: E402
import tricolour.packing as packing  # noqa: E402
import tricolour.stokes as stokes  # noqa: E402
import tricolour.mask as mask  # noqa: E402
import tricolour.window_statistics as ws  # noqa: E402
from tricolour.apps.tricolour.strat_executor import StrategyExecutor  # noqa: E402

NA, NTIME, NCHAN, NCORR = 8, 48, 64, 4
CORR_TYPE = [9, 10, 11, 12]         # XX XY YX YY
STRATEGIES = [
    {"name": "flag_autos", "task": "flag_autos"},
    {"name": "small_st", "task": "sum_threshold",
     "kwargs": {"outlier_nsigma": 4.5, "windows_time": [1, 2, 4], "windows_freq": [1, 2, 4],
                "background_reject": 2.0, "background_iterations": 1, "spike_width_time": 6.5,
                "spike_width_freq": 10.0, "time_extend": 3, "freq_extend": 3, "freq_chunks": 3,
                "average_freq": 1, "flag_all_time_frac": 0.6, "flag_all_freq_frac": 0.8, "rho": 1.3,
                "num_major_iterations": 1}},
    {"name": "combine_with_input_flags", "task": "combine_with_input_flags"},
    {"name": "static_mask", "task": "apply_static_mask",
     "kwargs": {"accumulation_mode": "or", "uvrange": "0~100"}},
]
CASES = [  # name, flagging strategy, model, ignore_flags, mask dilation
    ("standard_model", "standard", True, False, "2"),
    ("polarisation_model", "polarisation", True, False, "500kHz"),
    ("total_power", "total_power", False, False, "2"),
    ("standard_ignore_flags", "standard", True, True, "500kHz"),
]
ROW_COLUMNS = ("ant1", "ant2", "time", "data", "model", "flag")
STAT_FIELDS = ("counts_per_ant", "size_per_ant", "counts_per_bl", "size_per_bl", "counts_per_field",
               "size_per_field", "counts_per_scan", "size_per_scan", "counts_per_ddid", "bins_per_ddid",
               "size_per_ddid")


def plain(stats):
    return {f: {str(k): (np.asarray(v).tolist() if isinstance(v, np.ndarray) else int(v))
                for k, v in getattr(stats, "_" + f).items()} for f in STAT_FIELDS}


def make_rows(rs):
    a1, a2 = np.triu_indices(NA, 0)                      # autocorrelations included
    nbl = len(a1)
    times = 4.9e9 + 8.0 * np.arange(NTIME)
    ant1 = np.tile(a1, NTIME).astype(np.int32)
    ant2 = np.tile(a2, NTIME).astype(np.int32)
    tm = np.repeat(times, nbl)
    keep = rs.uniform(size=ant1.size) >= 0.03          # a few missing rows
    idx = np.nonzero(keep)[0]
    dup = rs.choice(idx, 6, replace=False)              # a few duplicated rows
    idx = rs.permutation(np.concatenate([idx, dup]))
    ant1, ant2, tm = ant1[idx], ant2[idx], tm[idx]
    shape = (ant1.size, NCHAN, NCORR)
    # values on a 1/64 grid: exact in complex64 and compressible, keeps the .npz small
    data = (np.round(64 * rs.standard_normal(shape)) + 1j * np.round(64 * rs.standard_normal(shape))) / 64
    data = data.astype(np.complex64)
    data[:, 17, :] += 12.0                               # a narrow-band RFI line
    data[rs.uniform(size=ant1.size) < 0.02, 40:44, :] *= 9.0
    data[5, 3, 1] = np.nan
    model = ((np.round(32 * rs.standard_normal(shape)) + 1j * np.round(32 * rs.standard_normal(shape))) / 64
             ).astype(np.complex64)
    flag = rs.uniform(size=shape) < 0.02
    flag[:, 60:62, 2] = True
    return ant1, ant2, tm, data, model, flag


def write_mask(path, rs):
    # a static mask on its own channel grid (~200 kHz), covering part of the band
    chans = np.linspace(1.30e9, 1.34e9, 201)
    m = np.zeros(chans.size, bool)
    m[[0, 1, 30, 31, 32, 90, 150, 200]] = True
    arr = np.zeros((2, chans.size), dtype=[("mask", bool), ("chans", np.float64)])
    arr["mask"][0] = m
    arr["chans"][1] = chans
    np.save(path, arr)
    return m, chans


def run_case(name, strategy, use_model, ignore_flags, masked_channels, rows, chan_freq, chan_width,
             antspos, antsnames, scan_no, field_name, ddid):
    ant1, ant2, tm, data, model, flag = rows
    nrow, nchan, ncorr = data.shape
    chunks = 97
    vis = da.from_array(data, chunks=(chunks, nchan, ncorr))
    if use_model:                                                            # app.py:389-395
        vis = vis - da.from_array(model, chunks=(chunks, nchan, ncorr))
    antenna1 = da.from_array(ant1, chunks=chunks)
    antenna2 = da.from_array(ant2, chunks=chunks)
    if ignore_flags:                                                         # :403-410
        flags = da.full_like(vis, False, dtype=bool)
    else:
        flags = da.from_array(flag, chunks=(chunks, nchan, ncorr))
    if strategy in ("polarisation", "total_power"):                          # :415-439
        stokes_map = stokes.stokes_corr_map(CORR_TYPE)
        stokes_pol = tuple(v for k, v in stokes_map.items() if strategy == "total_power" or k != "I")
        # numba's typing of the jitted loop: terms in complex128, result cast to the
        # visibility dtype (un-jitted NumPy would stay in complex64)
        vis = da.blockwise(lambda v: stokes.polarised_intensity(v.astype(np.complex128), stokes_pol)
                           .astype(v.dtype), ("row", "chan", "corr"), vis, ("row", "chan", "corr"),
                           adjust_chunks={"corr": 1}, dtype=vis.dtype)
        flags = da.any(flags, axis=2, keepdims=True)
    ubl = packing.unique_baselines(antenna1, antenna2)                       # :441-450
    utime, time_inv = da.unique(da.from_array(tm, chunks=chunks), return_inverse=True)
    utime, ubl = dask.compute(utime, ubl)
    ubl = ubl.view(np.int32).reshape(-1, 2)
    ubl = np.concatenate([np.arange(ubl.shape[0], dtype=ubl.dtype)[:, None], ubl], axis=1)
    ubl = da.from_array(ubl, chunks=(11, 3))
    vis_windows, flag_windows = packing.pack_data(time_inv, ubl, antenna1, antenna2, vis, flags,
                                                  utime.shape[0], backend="numpy")
    original = ws.window_stats(flag_windows, ubl, chan_freq, antsnames, scan_no, field_name, ddid)
    with StrategyExecutor(antspos, ubl, chan_freq, chan_width, masked_channels, STRATEGIES) as se:
        flag_windows = se.apply_strategies(flag_windows, vis_windows)
    final = ws.window_stats(flag_windows, ubl, chan_freq, antsnames, scan_no, field_name, ddid)
    unpacked = packing.unpack_data(antenna1, antenna2, time_inv, ubl, flag_windows)   # :475-480
    equalized = da.sum(unpacked, axis=2, keepdims=True) > 0
    corr_flags = da.broadcast_to(equalized, (nrow, nchan, ncorr))
    out, orig, fin = dask.compute(corr_flags, original, final, scheduler="single-threaded")
    return out, orig, fin


def main():
    t0 = time.time()
    rs = np.random.RandomState(15)
    rows = make_rows(rs)       # keep in step with _g15_rows in tests/test_scan_gpu.py
    chan_freq = np.linspace(1.300e9, 1.338e9, NCHAN)
    chan_width = np.full(NCHAN, chan_freq[1] - chan_freq[0])
    antspos = np.stack([rs.uniform(-150, 150, NA), rs.uniform(-150, 150, NA), np.zeros(NA)], axis=1) + \
        np.array([5109e3, 2006e3, -3238e3])
    antsnames = ["m%03d" % i for i in range(NA)]
    scan_no, field_name, ddid = 3, "J1939-6342", 0
    # the MS columns are not stored: tests/test_scan_gpu.py rebuilds them with the same make_rows
    # (legacy RandomState streams are fixed across numpy versions) and checks these digests
    arrays = dict(rows_seed=np.int64(15), rows_shape=np.array([NA, NTIME, NCHAN, NCORR], np.int64),
                  rows_sha256=np.array(json.dumps({k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()
                                                   for k, v in zip(ROW_COLUMNS, rows)})),
                  chan_freq=chan_freq, chan_width=chan_width, antspos=antspos, antsnames=np.array(antsnames),
                  corr_type=np.array(CORR_TYPE, np.int32), strategies=np.array(json.dumps(STRATEGIES)),
                  call=np.array(json.dumps([scan_no, field_name, ddid])))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "band.staticmask")
        with open(path, "wb") as fh:
            m, chans = write_mask(fh, rs)
        arrays.update(mask_flags=m, mask_chans=chans)
        dilations = ["2", "500kHz", "0", "40", "1", "0.2MHz", "1000Hz"]
        masked = {}
        for dil in dilations:
            masked[dil] = mask.load_mask(path, dil)
            arrays["masked_channels_" + dil] = masked[dil]
            arrays["dilated_" + dil] = mask.dilate_mask(chans, m, dil)
        arrays["masked_channels_none"] = mask.load_mask(path, None)
        arrays["dilations"] = np.array(json.dumps(dilations))
        doc = []
        for name, strategy, use_model, ignore_flags, dil in CASES:
            out, orig, fin = run_case(name, strategy, use_model, ignore_flags, [masked[dil]], rows,
                                      chan_freq, chan_width, antspos, antsnames, scan_no, field_name, ddid)
            # the application broadcasts one flag per (row, chan) to every correlation (app.py:479-480):
            # keep that one, bit-packed
            assert (out == out[..., :1]).all()
            arrays["flags_" + name] = np.packbits(out[..., 0], axis=None)
            doc.append({"name": name, "strategy": strategy, "model": use_model, "ignore_flags": ignore_flags,
                        "dilate": dil, "original": plain(orig), "final": plain(fin)})
            print("%s: %d of %d flagged" % (name, out.sum(), out.size), flush=True)
        arrays["cases"] = np.array(json.dumps(doc))
    np.savez_compressed("G15_scan.npz", **arrays)
    print("G15 written (%.0f s)" % (time.time() - t0))


if __name__ == "__main__":
    main()
