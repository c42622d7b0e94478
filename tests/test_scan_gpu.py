"""Whole-scan flagging on the device: flag_scan against the reference
application's per-scan steps (G15), the fused scan pack against the
unfused kernels it replaces, the broadcast unpack against numpy, and a
larger randomised scan against the composed existing calls."""
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


@pytest.mark.gpu
@pytest.mark.parametrize("name", _g15_cases())
def test_gpu_flag_scan_matches_reference_application(gpu, name):
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
        antenna_names=list(d["antsnames"]), scan_no=scan_no, field_name=field_name, ddid=ddid)
    exp = g15_row_flags(d, name, r)
    assert isinstance(flags, np.ndarray) and flags.dtype == np.bool_ and flags.shape == exp.shape
    nbad = int((flags != exp).sum())
    assert nbad == 0, "%d of %d flags differ from the reference" % (nbad, exp.size)
    assert _plain(original) == case["original"]
    assert _plain(final) == case["final"]


@pytest.mark.gpu
def test_gpu_flag_scans_loop_and_summary(gpu):
    """Two copies of the G15 scan as two fields: the field / scan selection
    and the combined summary of the loop; tensors stay on the device."""
    import torch
    from tricolour_amd import scan
    from tricolour_amd.window_statistics import summarise_stats
    d, _ = load_golden("G15_scan.npz")
    case = json.loads(str(d["cases"]))[0]
    strategies = json.loads(str(d["strategies"]))
    r = g15_rows(d)
    common = dict(DATA=torch.from_numpy(r["data"]).cuda(), FLAG=torch.from_numpy(r["flag"]).cuda(),
                  MODEL=torch.from_numpy(r["model"]).cuda(), ANTENNA1=r["ant1"], ANTENNA2=r["ant2"],
                  TIME=r["time"], CHAN_FREQ=d["chan_freq"], CHAN_WIDTH=d["chan_width"], DATA_DESC_ID=0)
    datasets = [dict(common, FIELD_ID=0, SCAN_NUMBER=1), dict(common, FIELD_ID=1, SCAN_NUMBER=2),
                dict(common, FIELD_ID=1, SCAN_NUMBER=3)]
    kw = dict(fieldnames=["A", "B"], antenna_positions=d["antspos"], antenna_names=list(d["antsnames"]),
              masked_channels=[d["masked_channels_" + case["dilate"]]])
    out, summary = scan.flag_scans(datasets, strategies, scan_numbers=[1, 2], field_names=["1"], **kw)
    assert out[0] is None and out[2] is None
    assert torch.is_tensor(out[1]) and out[1].is_cuda
    assert np.array_equal(out[1].cpu().numpy(), g15_row_flags(d, case["name"], r))
    _, original, final = scan.flag_scan(
        common["DATA"], common["FLAG"], r["ant1"], r["ant2"], r["time"], d["chan_freq"], d["chan_width"],
        strategies, model=common["MODEL"], antenna_positions=d["antspos"], antenna_names=list(d["antsnames"]),
        masked_channels=kw["masked_channels"], scan_no=2, field_name="B", ddid=0)
    assert summary == summarise_stats(final, original)
    out, summary = scan.flag_scans(datasets, strategies, scan_numbers=[7], **kw)
    assert out == [None, None, None] and summary == []


def _rows(rs, na, ntime, nchan, ncorr, delete_frac=0.05, ndup=5, extra_bl=False):
    a1, a2 = np.triu_indices(na, 0)
    nbl = len(a1)
    ant1 = np.tile(a1, ntime).astype(np.int32)
    ant2 = np.tile(a2, ntime).astype(np.int32)
    tinv = np.repeat(np.arange(ntime), nbl).astype(np.int32)
    idx = np.nonzero(rs.uniform(size=ant1.size) >= delete_frac)[0]
    idx = rs.permutation(np.concatenate([idx, rs.choice(idx, ndup, replace=False)]))
    ant1, ant2, tinv = ant1[idx], ant2[idx], tinv[idx]
    shape = (ant1.size, nchan, ncorr)
    data = (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(np.complex64)
    model = (0.3 * rs.standard_normal(shape) + 0.3j * rs.standard_normal(shape)).astype(np.complex64)
    flag = rs.uniform(size=shape) < 0.1
    from tricolour_amd import packing
    ubl = packing.unique_baselines(ant1, ant2)
    if extra_bl:   # windows of a baseline chunk: rows of the other baselines map nowhere
        ubl = ubl[::2].copy()
        ubl[:, 0] = np.arange(ubl.shape[0])
    return ant1, ant2, tinv, ubl, data, model, flag


def _same_windows(vw, fw, ev, ef):
    a, b = vw.cpu().numpy(), ev.cpu().numpy()
    assert a.shape == b.shape
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))        # bit-identical, NaN fill included
    assert np.array_equal(fw.cpu().numpy(), ef.cpu().numpy())


PACK_CASES = [
    # na, ntime, nchan, ncorr, corr names
    (5, 7, 37, 4, ["XX", "XY", "YX", "YY"]),
    (4, 5, 64, 4, ["RR", "RL", "LR", "LL"]),
    (4, 6, 13, 2, ["XX", "YY"]),
    (3, 4, 9, 1, None),
    (4, 3, 11, 3, ["XX", "XY", "YY"]),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", PACK_CASES)
@pytest.mark.parametrize("strategy", ["standard", "polarisation", "total_power"])
@pytest.mark.parametrize("with_model", [True, False])
@pytest.mark.parametrize("extra_bl", [False, True])
def test_gpu_pack_scan_matches_unfused_kernels(gpu, case, strategy, with_model, extra_bl):
    import torch
    from tricolour_amd import packing, stokes
    na, ntime, nchan, ncorr, names = case
    if strategy != "standard" and names is None:
        pytest.skip("one correlation forms no Stokes parameter")
    rs = np.random.RandomState(nchan * 10 + ncorr)
    ant1, ant2, tinv, ubl, data, model, flag = _rows(rs, na, ntime, nchan, ncorr, extra_bl=extra_bl)
    data[2, 3, 0] = np.nan
    d, m, f = (torch.from_numpy(x).cuda() for x in (data, model, flag))
    terms = ()
    if strategy != "standard":
        cmap = stokes.stokes_corr_map([stokes.STOKES_TYPES[n] for n in names])
        terms = tuple(v for k, v in cmap.items() if strategy == "total_power" or k != "I")
        if not terms:
            pytest.skip("no polarised terms")
    vw, fw = packing.pack_scan(tinv, ubl, ant1, ant2, d, f, ntime, model=m if with_model else None,
                               flagging_strategy=strategy, stokes_terms=terms)
    resid = d - m if with_model else d
    if strategy == "standard":
        ev, ef = packing.pack_data(tinv, ubl, ant1, ant2, resid, f, ntime)
    else:
        inten = stokes.polarised_intensity(resid, terms)
        ev, ef = packing.pack_data(tinv, ubl, ant1, ant2, inten, f.any(dim=2, keepdim=True), ntime)
    torch.cuda.synchronize()
    _same_windows(vw, fw, ev, ef)
    # --ignore-flags: mapped cells unflagged, unmapped cells keep the fill
    vw0, fw0 = packing.pack_scan(tinv, ubl, ant1, ant2, d, None, ntime, model=m if with_model else None,
                                 flagging_strategy=strategy, stokes_terms=terms)
    _, ef0 = packing.pack_data(tinv, ubl, ant1, ant2, resid[..., :ef.shape[1]],
                               torch.zeros(resid.shape[:2] + (ef.shape[1],), dtype=torch.bool, device=d.device),
                               ntime)
    _same_windows(vw0, fw0, vw, ef0)


@pytest.mark.gpu
@pytest.mark.parametrize("wcorr,ncorr", [(1, 4), (4, 4), (1, 1), (2, 2), (1, 3), (3, 3)])
@pytest.mark.parametrize("extra_bl", [False, True])
def test_gpu_unpack_scan_matches_numpy(gpu, wcorr, ncorr, extra_bl):
    import torch
    from tricolour_amd import packing
    rs = np.random.RandomState(wcorr * 7 + ncorr)
    nchan, ntime = 45, 6
    ant1, ant2, tinv, ubl, _, _, _ = _rows(rs, 5, ntime, nchan, 1, extra_bl=extra_bl)
    fw = rs.uniform(size=(ubl.shape[0], wcorr, ntime, nchan)) < 0.2
    out = packing.unpack_scan(ant1, ant2, tinv, ubl, torch.from_numpy(fw).cuda(), ncorr).cpu().numpy()
    row_bl, _, row_time = packing.row_map(ant1, ant2, ubl, tinv, ntime)
    exp = np.zeros((ant1.size, nchan, ncorr), bool)
    ok = row_bl >= 0
    anyc = fw.any(axis=1)                                    # (bl, time, chan)
    exp[ok] = anyc[row_bl[ok], row_time[ok]][:, :, None]
    assert out.dtype == np.bool_ and np.array_equal(out, exp)
    if wcorr > 1:   # windows of several correlations only go back to as many
        with pytest.raises(ValueError):
            packing.unpack_scan(ant1, ant2, tinv, ubl, torch.from_numpy(fw).cuda(), ncorr + 1)


@pytest.mark.gpu
def test_gpu_flag_scan_large_polarisation_matches_composed_calls(gpu):
    """64 antennas x 256 times x 1024 channels, polarisation mode: flag_scan
    against stokes -> pack_data -> apply_strategies -> unpack_data and the
    numpy broadcast."""
    import torch
    from tricolour_amd import packing, scan, stokes
    from tricolour_amd.strategies import apply_strategies
    rs = np.random.RandomState(64)
    na, ntime, nchan = 64, 256, 1024
    a1, a2 = np.triu_indices(na, 1)
    nbl = len(a1)
    ant1 = np.tile(a1, ntime).astype(np.int32)
    ant2 = np.tile(a2, ntime).astype(np.int32)
    tm = np.repeat(1e9 + 2.0 * np.arange(ntime), nbl)
    shape = (ant1.size, nchan, 4)
    g = torch.Generator(device="cuda").manual_seed(64)
    data = torch.randn(shape, dtype=torch.complex64, device="cuda", generator=g)
    model = 0.1 * torch.randn(shape, dtype=torch.complex64, device="cuda", generator=g)
    data[:, 300, :] += 20.0
    flags = torch.rand(shape, device="cuda", generator=g) < 0.01
    strategies = [{"task": "flag_autos"},
                  {"task": "sum_threshold", "kwargs": {"outlier_nsigma": 5.0, "windows_time": [1, 2, 4],
                                                       "windows_freq": [1, 2, 4], "num_major_iterations": 1,
                                                       "background_iterations": 1}},
                  {"task": "combine_with_input_flags"}]
    corr = [9, 10, 11, 12]
    got, _, _ = scan.flag_scan(data, flags, ant1, ant2, tm, np.linspace(1e9, 1.1e9, nchan), np.full(nchan, 1e5),
                               strategies, model=model, flagging_strategy="polarisation", corr_type=corr)
    assert got.is_cuda and got.shape == shape
    terms = tuple(v for k, v in stokes.stokes_corr_map(corr).items() if k != "I")
    inten = stokes.polarised_intensity(data - model, terms)
    ubl = packing.unique_baselines(ant1, ant2)
    _, tinv = np.unique(tm, return_inverse=True)
    vw, fw = packing.pack_data(tinv, ubl, ant1, ant2, inten, flags.any(dim=2, keepdim=True), ntime)
    fw = apply_strategies(strategies, fw, vw, ubl=ubl)
    up = packing.unpack_data(ant1, ant2, tinv, ubl, fw)
    exp = up.any(dim=2, keepdim=True).expand(shape)
    assert int((got != exp).sum()) == 0
    assert 0 < int(got.sum()) < got.numel()
