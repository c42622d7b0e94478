"""Baseline-chunked scans on the device: flag_scan(..., baseline_chunks=N)
against the reference application (G15) and against the whole-scan path, the
row-list pack / unpack kernels against their whole-scan siblings, and the
device memory a streamed host scan holds."""
import json

import numpy as np
import pytest

from conftest import load_golden
from test_scan_host import g15_row_flags, g15_rows

STAT_FIELDS = ("counts_per_ant", "size_per_ant", "counts_per_bl", "size_per_bl", "counts_per_field",
               "size_per_field", "counts_per_scan", "size_per_scan", "counts_per_ddid", "bins_per_ddid",
               "size_per_ddid")


def _plain(stats):
    return {f: {str(k): (np.asarray(v).tolist() if isinstance(v, np.ndarray) else int(v))
                for k, v in getattr(stats, "_" + f).items()} for f in STAT_FIELDS}


def _g15_cases():
    d, _ = load_golden("G15_scan.npz")
    return [c["name"] for c in json.loads(str(d["cases"]))]


# ---------------------------------------------------------------------------
# G15: the reference application's flags and tallies, chunked
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5, 16, 36])
@pytest.mark.parametrize("name", _g15_cases())
def test_gpu_chunked_flag_scan_matches_reference_application(gpu, name, n):
    from tricolour_amd import scan
    d, _ = load_golden("G15_scan.npz")
    case = {c["name"]: c for c in json.loads(str(d["cases"]))}[name]
    scan_no, field_name, ddid = json.loads(str(d["call"]))
    r = g15_rows(d)
    flags, original, final = scan.flag_scan(
        r["data"], r["flag"], r["ant1"], r["ant2"], r["time"], d["chan_freq"], d["chan_width"],
        json.loads(str(d["strategies"])), model=r["model"] if case["model"] else None,
        flagging_strategy=case["strategy"], corr_type=d["corr_type"], ignore_flags=case["ignore_flags"],
        antenna_positions=d["antspos"], masked_channels=[d["masked_channels_" + case["dilate"]]],
        antenna_names=list(d["antsnames"]), scan_no=scan_no, field_name=field_name, ddid=ddid,
        baseline_chunks=n)
    assert scan.last_stream_stats()["chunks"] == -(-36 // n)
    exp = g15_row_flags(d, name, r)
    assert isinstance(flags, np.ndarray) and flags.dtype == np.bool_ and flags.shape == exp.shape
    nbad = int((flags != exp).sum())
    assert nbad == 0, "%d of %d flags differ from the reference" % (nbad, exp.size)
    assert _plain(original) == case["original"]
    assert _plain(final) == case["final"]


@pytest.mark.gpu
@pytest.mark.parametrize("on_device", [False, True])
def test_gpu_chunked_flag_scans_matches_whole_scans(gpu, on_device):
    import torch
    from tricolour_amd import scan
    d, _ = load_golden("G15_scan.npz")
    case = json.loads(str(d["cases"]))[0]
    strategies = json.loads(str(d["strategies"]))
    r = g15_rows(d)
    cols = {k: (torch.from_numpy(r[k]).cuda() if on_device else r[k]) for k in ("data", "flag", "model")}
    common = dict(DATA=cols["data"], FLAG=cols["flag"], MODEL=cols["model"], ANTENNA1=r["ant1"],
                  ANTENNA2=r["ant2"], TIME=r["time"], CHAN_FREQ=d["chan_freq"], CHAN_WIDTH=d["chan_width"],
                  DATA_DESC_ID=0)
    datasets = [dict(common, FIELD_ID=0, SCAN_NUMBER=1), dict(common, FIELD_ID=1, SCAN_NUMBER=2),
                dict(common, FIELD_ID=1, SCAN_NUMBER=3)]
    kw = dict(fieldnames=["A", "B"], antenna_positions=d["antspos"], antenna_names=list(d["antsnames"]),
              masked_channels=[d["masked_channels_" + case["dilate"]]])
    whole, whole_summary = scan.flag_scans(datasets, strategies, scan_numbers=[1, 2, 3], **kw)
    chunked, chunked_summary = scan.flag_scans(datasets, strategies, scan_numbers=[1, 2, 3], baseline_chunks=7,
                                               **kw)
    assert chunked_summary == whole_summary and len(whole_summary) > 10
    for w, c in zip(whole, chunked):
        if on_device:
            assert torch.is_tensor(c) and c.is_cuda and c.dtype == torch.bool
            w, c = w.cpu().numpy(), c.cpu().numpy()
        else:
            assert isinstance(c, np.ndarray) and c.dtype == np.bool_
        assert np.array_equal(w, c)
    assert np.array_equal(chunked[1] if not on_device else chunked[1].cpu().numpy(),
                          g15_row_flags(d, case["name"], r))


# ---------------------------------------------------------------------------
# row-list kernels against the whole-scan kernels
# ---------------------------------------------------------------------------
def _rows(rs, na, ntime, nchan, ncorr):
    a1, a2 = np.triu_indices(na, 0)
    nbl = len(a1)
    ant1 = np.tile(a1, ntime).astype(np.int32)
    ant2 = np.tile(a2, ntime).astype(np.int32)
    tinv = np.repeat(np.arange(ntime), nbl).astype(np.int32)
    idx = np.nonzero(rs.uniform(size=ant1.size) >= 0.1)[0]
    idx = rs.permutation(np.concatenate([idx, rs.choice(idx, 6, replace=False)]))
    ant1, ant2, tinv = ant1[idx], ant2[idx], tinv[idx]
    shape = (ant1.size, nchan, ncorr)
    data = (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(np.complex64)
    data[3, nchan // 2, 0] = np.nan
    model = (0.3 * rs.standard_normal(shape) + 0.3j * rs.standard_normal(shape)).astype(np.complex64)
    flag = rs.uniform(size=shape) < 0.1
    return ant1, ant2, tinv, data, model, flag


CORR_NAMES = {1: None, 2: ["XX", "YY"], 3: ["XX", "XY", "YY"], 4: ["XX", "XY", "YX", "YY"]}


def _terms(strategy, ncorr):
    from tricolour_amd import stokes
    if strategy == "standard":
        return ()
    names = CORR_NAMES[ncorr]
    if names is None:
        return None
    cmap = stokes.stokes_corr_map([stokes.STOKES_TYPES[n] for n in names])
    return tuple(v for k, v in cmap.items() if strategy == "total_power" or k != "I") or None


def _windows(torch, nbl, wcorr, ntime, nchan):
    from tricolour_amd import _lib
    vw = torch.empty((nbl, wcorr, ntime, nchan), dtype=torch.complex64, device="cuda")
    fw = torch.empty((nbl, wcorr, ntime, nchan), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().tri_fill_windows(vw.data_ptr(), fw.data_ptr(), vw.numel(),
                                           torch.cuda.current_stream().cuda_stream))
    return vw, fw


def _misaligned(torch, t):
    """t's values at an address 8 bytes past a 16-byte boundary: the scalar kernel's input."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    flat[1:].copy_(t.reshape(-1))
    out = flat[1:].view(t.shape)
    assert out.data_ptr() % 16 != 0
    return out


# (ncorr, strategy) pairs whose correlations form the strategy's Stokes parameters
PACK_MODES = [(nc, st) for nc in (1, 2, 3, 4) for st in ("standard", "polarisation", "total_power")
              if _terms(st, nc) is not None]


@pytest.mark.gpu
@pytest.mark.parametrize("nchan", [37, 64])
@pytest.mark.parametrize("ncorr,strategy", PACK_MODES)
@pytest.mark.parametrize("with_model,with_flags", [(True, True), (False, True), (True, False), (False, False)])
def test_gpu_pack_scan_rows_matches_pack_scan(gpu, nchan, ncorr, strategy, with_model, with_flags):
    import torch
    from tricolour_amd import packing
    terms = _terms(strategy, ncorr)
    rs = np.random.RandomState(nchan * 10 + ncorr)
    na, ntime = 6, 5
    ant1, ant2, tinv, data, model, flag = _rows(rs, na, ntime, nchan, ncorr)
    ubl = packing.unique_baselines(ant1, ant2)
    d = torch.from_numpy(data).cuda()
    m = torch.from_numpy(model).cuda() if with_model else None
    f = torch.from_numpy(flag).cuda() if with_flags else None
    ev, ef = packing.pack_scan(tinv, ubl, ant1, ant2, d, f, ntime, model=m, flagging_strategy=strategy,
                               stokes_terms=terms)
    f8 = None if f is None else f.view(torch.uint8)
    wcorr = ev.shape[1]

    def idx(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()

    chunks = list(packing.scan_chunks(ant1, ant2, ubl, tinv, ntime, 8))
    assert [c.b1 - c.b0 for c in chunks] == [8, 8, 5]
    for c in chunks:
        exp_v, exp_f = ev[c.b0:c.b1], ef[c.b0:c.b1].view(torch.uint8)
        nb = c.b1 - c.b0
        pb, pt = idx(c.bl[c.pack], np.int32), idx(c.time[c.pack], np.int32)
        # list entries -1: duplicates of a cell that an earlier row fills, skipped as row_map does
        bl_all = np.full(c.rows.size, -1, np.int32)
        bl_all[c.pack] = c.bl[c.pack]
        slab = [None if x is None else x[idx(c.rows, np.int64)].contiguous() for x in (d, m, f8)]
        variants = [
            ("scattered src_row", (d, m, f8), idx(c.pack_rows, np.int64), pb, pt),
            ("compact slab", slab, None, idx(bl_all, np.int32), idx(c.time, np.int32)),
            ("slab src_row", slab, idx(c.pack, np.int64), pb, pt),
            ("scalar path", [None if x is None else _misaligned(torch, x) for x in (d, m)] + [f8],
             idx(c.pack_rows, np.int64), pb, pt),
        ]
        for what, (dd, mm, ff), src, rb, rt in variants:
            vw, fw = _windows(torch, nb, wcorr, ntime, nchan)
            packing.pack_scan_rows(dd, mm, ff, src, rb, rt, nb, ntime, vw, fw, flagging_strategy=strategy,
                                   stokes_terms=terms)
            torch.cuda.synchronize()
            assert np.array_equal(vw.cpu().numpy().view(np.uint64), exp_v.cpu().numpy().view(np.uint64)), what
            assert np.array_equal(fw.cpu().numpy(), exp_f.cpu().numpy()), what


@pytest.mark.gpu
@pytest.mark.parametrize("wcorr,ncorr", [(1, 4), (4, 4), (1, 1), (2, 2), (1, 3), (3, 3)])
def test_gpu_unpack_scan_rows_matches_unpack_scan(gpu, wcorr, ncorr):
    import torch
    from tricolour_amd import packing
    rs = np.random.RandomState(wcorr * 7 + ncorr)
    nchan, ntime = 45, 6
    ant1, ant2, tinv, _, _, _ = _rows(rs, 6, ntime, 1, 1)
    ubl = packing.unique_baselines(ant1, ant2)
    fw = torch.from_numpy(rs.uniform(size=(ubl.shape[0], wcorr, ntime, nchan)) < 0.2).cuda()
    exp = packing.unpack_scan(ant1, ant2, tinv, ubl, fw, ncorr).view(torch.uint8).cpu().numpy()
    fw8 = fw.view(torch.uint8)
    for c in packing.scan_chunks(ant1, ant2, ubl, tinv, ntime, 8):
        rb = torch.from_numpy(c.bl).cuda()
        rt = torch.from_numpy(c.time).cuda()
        out = torch.full((ant1.size, nchan, ncorr), 7, dtype=torch.uint8, device="cuda")
        packing.unpack_scan_rows(fw8[c.b0:c.b1], torch.from_numpy(c.rows).cuda(), rb, rt, out)
        got = out.cpu().numpy()
        assert np.array_equal(got[c.rows], exp[c.rows])
        others = np.ones(ant1.size, bool)
        others[c.rows] = False
        assert np.all(got[others] == 7)
        compact = torch.full((c.rows.size, nchan, ncorr), 7, dtype=torch.uint8, device="cuda")
        packing.unpack_scan_rows(fw8[c.b0:c.b1], None, rb, rt, compact)
        assert np.array_equal(compact.cpu().numpy(), exp[c.rows])


# ---------------------------------------------------------------------------
# a randomised MeerKAT-like scan, chunked against whole
# ---------------------------------------------------------------------------
_BIG = {}


def _big_scan():
    """64 antennas with autos (2080 baselines) x 96 dumps x 512 channels x 4 correlations, with missing and
    duplicated rows in random order; drawn on the device (fixed seed)."""
    import torch
    if _BIG:
        return _BIG
    rs = np.random.RandomState(2080)
    na, ntime, nchan = 64, 96, 512
    a1, a2 = np.triu_indices(na, 0)
    nbl = len(a1)
    ant1 = np.tile(a1, ntime).astype(np.int32)
    ant2 = np.tile(a2, ntime).astype(np.int32)
    tm = np.repeat(4.9e9 + 8.0 * np.arange(ntime), nbl)
    idx = np.nonzero(rs.uniform(size=ant1.size) >= 0.02)[0]
    idx = np.concatenate([idx, rs.choice(idx, 50, replace=False)])
    idx = np.sort(idx, kind="stable")
    # mostly time-major, baseline-ordered rows; a few dumps shuffled
    for t in (5, 40):
        sel = np.nonzero((idx // nbl) == t)[0]
        idx[sel] = rs.permutation(idx[sel])
    ant1, ant2, tm = ant1[idx], ant2[idx], tm[idx]
    shape = (ant1.size, nchan, 4)
    g = torch.Generator(device="cuda").manual_seed(2080)
    data = torch.randn(shape, dtype=torch.complex64, device="cuda", generator=g)
    data[:, 100, :] += 15.0
    data[::97, 300:310, :] *= 8.0
    model = 0.2 * torch.randn(shape, dtype=torch.complex64, device="cuda", generator=g)
    flags = torch.rand(shape, device="cuda", generator=g) < 0.02
    antpos = rs.uniform(-4000, 4000, size=(na, 3))
    freq = np.linspace(0.856e9, 1.712e9, nchan)
    mask = freq[[50, 51, 52, 400]][:, None]
    _BIG.update(ant1=ant1, ant2=ant2, time=tm, data=data, model=model, flags=flags, antpos=antpos, freq=freq,
                width=np.full(nchan, freq[1] - freq[0]), mask=mask)
    return _BIG


BIG_STRATEGIES = [
    {"task": "uvcontsub_flagger", "kwargs": {"major_cycles": 2, "or_original_from_cycle": 0, "taylor_degrees": 8,
                                             "sigma": 5.0}},
    {"task": "sum_threshold", "kwargs": {"outlier_nsigma": 4.5, "windows_time": [1, 2, 4, 8],
                                         "windows_freq": [1, 2, 4, 8], "background_reject": 2.0,
                                         "background_iterations": 1, "spike_width_time": 6.5,
                                         "spike_width_freq": 10.0, "time_extend": 3, "freq_extend": 3,
                                         "freq_chunks": 4, "average_freq": 1, "flag_all_time_frac": 0.6,
                                         "flag_all_freq_frac": 0.8, "rho": 1.3, "num_major_iterations": 2}},
    {"task": "flag_autos"},
    {"task": "apply_static_mask", "kwargs": {"accumulation_mode": "or", "uvrange": "0~3000"}},
    {"task": "combine_with_input_flags"},
]


@pytest.mark.gpu
@pytest.mark.parametrize("strategy", ["standard", "polarisation", "total_power"])
def test_gpu_chunked_random_scan_matches_whole_scan(gpu, strategy):
    import torch
    from tricolour_amd import scan
    s = _big_scan()
    kw = dict(model=s["model"], flagging_strategy=strategy, corr_type=["XX", "XY", "YX", "YY"],
              antenna_positions=s["antpos"], masked_channels=[s["mask"]], scan_no=3, field_name="F", ddid=1)
    args = (s["ant1"], s["ant2"], s["time"], s["freq"], s["width"], BIG_STRATEGIES)
    whole, w_orig, w_final = scan.flag_scan(s["data"], s["flags"], *args, **kw)
    exp = whole.cpu().numpy()
    assert 0 < exp.sum() < exp.size
    host = dict(kw, model=s["model"].cpu().numpy())
    data_h, flags_h = s["data"].cpu().numpy(), s["flags"].cpu().numpy()
    for n in (7, 500):
        got, orig, final = scan.flag_scan(data_h, flags_h, *args, baseline_chunks=n, **host)
        assert isinstance(got, np.ndarray) and got.dtype == np.bool_
        nbad = int((got != exp).sum())
        assert nbad == 0, "numpy, N=%d: %d flags differ" % (n, nbad)
        assert _plain(orig) == _plain(w_orig) and _plain(final) == _plain(w_final)
        got, orig, final = scan.flag_scan(s["data"], s["flags"], *args, baseline_chunks=n, **kw)
        assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.bool
        nbad = int((got.cpu().numpy() != exp).sum())
        assert nbad == 0, "device, N=%d: %d flags differ" % (n, nbad)
        assert _plain(orig) == _plain(w_orig) and _plain(final) == _plain(w_final)


# ---------------------------------------------------------------------------
# device memory of a streamed host scan
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_chunked_host_scan_holds_a_fraction_of_the_device_memory(gpu):
    import torch
    from tricolour_amd import flagging, scan
    rs = np.random.RandomState(63)
    na, ntime, nchan = 63, 16, 64                   # 2016 baselines with autos
    a1, a2 = np.triu_indices(na, 0)
    nbl = len(a1)
    ant1 = np.tile(a1, ntime).astype(np.int32)
    ant2 = np.tile(a2, ntime).astype(np.int32)
    tm = np.repeat(1e9 + 8.0 * np.arange(ntime), nbl)
    shape = (ant1.size, nchan, 4)
    data = (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(np.complex64)
    model = (0.1 * rs.standard_normal(shape)).astype(np.complex64)
    flags = rs.uniform(size=shape) < 0.02
    strategies = [{"task": "sum_threshold", "kwargs": {"windows_time": [1, 2, 4], "windows_freq": [1, 2, 4],
                                                       "num_major_iterations": 1}},
                  {"task": "flag_autos"}, {"task": "combine_with_input_flags"}]
    args = (data, flags, ant1, ant2, tm, np.linspace(1e9, 1.1e9, nchan), np.full(nchan, 1e5), strategies)
    peaks, results = [], []
    for n in (None, 64):
        flagging.release_workspace()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        got, _, _ = scan.flag_scan(*args, model=model, baseline_chunks=n)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
        results.append(got.cpu().numpy() if torch.is_tensor(got) else got)
    assert np.array_equal(results[0], results[1])
    assert peaks[1] < peaks[0] / 4, "peak device memory: whole %d B, N=64 %d B" % tuple(peaks)
