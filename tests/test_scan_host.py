"""Whole-scan flagging, host side: static masks (mask.py:24-90) against the
reference's own load_mask / dilate_mask (G15), strategy YAML loading, the
field and scan selection of app.py:327-368, flag_scan's argument checks and
the two new C-ABI entry points.  No GPU needed."""
import hashlib
import json

import numpy as np
import pytest

from conftest import load_golden


def g15_rows(d):
    """The MS columns of G15 (ant1, ant2, time, data, model, flag), rebuilt as
    make_golden_scan.make_rows draws them from the stored seed; the fixture
    keeps their sha256 digests instead of the arrays."""
    na, ntime, nchan, ncorr = (int(v) for v in d["rows_shape"])
    rs = np.random.RandomState(int(d["rows_seed"]))
    a1, a2 = np.triu_indices(na, 0)
    nbl = len(a1)
    times = 4.9e9 + 8.0 * np.arange(ntime)
    ant1 = np.tile(a1, ntime).astype(np.int32)
    ant2 = np.tile(a2, ntime).astype(np.int32)
    tm = np.repeat(times, nbl)
    keep = rs.uniform(size=ant1.size) >= 0.03
    idx = np.nonzero(keep)[0]
    dup = rs.choice(idx, 6, replace=False)
    idx = rs.permutation(np.concatenate([idx, dup]))
    ant1, ant2, tm = ant1[idx], ant2[idx], tm[idx]
    shape = (ant1.size, nchan, ncorr)
    data = (np.round(64 * rs.standard_normal(shape)) + 1j * np.round(64 * rs.standard_normal(shape))) / 64
    data = data.astype(np.complex64)
    data[:, 17, :] += 12.0
    data[rs.uniform(size=ant1.size) < 0.02, 40:44, :] *= 9.0
    data[5, 3, 1] = np.nan
    model = ((np.round(32 * rs.standard_normal(shape)) + 1j * np.round(32 * rs.standard_normal(shape))) / 64
             ).astype(np.complex64)
    flag = rs.uniform(size=shape) < 0.02
    flag[:, 60:62, 2] = True
    rows = dict(ant1=ant1, ant2=ant2, time=tm, data=data, model=model, flag=flag)
    digests = json.loads(str(d["rows_sha256"]))
    for k, v in rows.items():
        assert hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() == digests[k], \
            "G15 column %s does not rebuild from its seed" % k
    return rows


def g15_row_flags(d, name, rows):
    """Reference row flags of a G15 case, (row, chan, corr): one bit-packed flag
    per (row, chan), broadcast over corr as the application writes them."""
    nrow, nchan, ncorr = rows["data"].shape
    one = np.unpackbits(d["flags_" + name], count=nrow * nchan).astype(bool).reshape(nrow, nchan, 1)
    return np.broadcast_to(one, (nrow, nchan, ncorr))


def test_g15_rows_rebuild_from_seed():
    d, _ = load_golden("G15_scan.npz")
    rows = g15_rows(d)
    assert rows["data"].shape == rows["model"].shape == rows["flag"].shape
    assert np.isnan(rows["data"]).any() and rows["flag"].any()
    for case in json.loads(str(d["cases"])):
        got = g15_row_flags(d, case["name"], rows)
        assert 0 < got.sum() < got.size


def _write_mask(path, flags, chans):
    arr = np.zeros((2, chans.size), dtype=[("mask", bool), ("chans", np.float64)])
    arr["mask"][0] = flags
    arr["chans"][1] = chans
    with open(path, "wb") as fh:
        np.save(fh, arr)


def test_scan_entry_points_are_exported():
    from tricolour_amd import _lib
    lib = _lib.lib()
    for name in ("tri_pack_scan", "tri_unpack_scan"):
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)


def test_dilate_and_load_mask_match_reference(tmp_path):
    from tricolour_amd import scan
    d, _ = load_golden("G15_scan.npz")
    flags, chans = d["mask_flags"], d["mask_chans"]
    path = str(tmp_path / "band.staticmask")
    _write_mask(path, flags, chans)
    for dil in json.loads(str(d["dilations"])):
        got = scan.dilate_mask(chans, flags, dil)
        assert got.dtype == np.bool_
        assert np.array_equal(got, d["dilated_" + dil]), dil
        masked = scan.load_mask(path, dil)
        assert masked.shape == d["masked_channels_" + dil].shape
        assert np.array_equal(masked, d["masked_channels_" + dil]), dil
    assert np.array_equal(scan.load_mask(path, None), d["masked_channels_none"])


@pytest.mark.parametrize("n", [0, 1, 2, 3, 7, 50, 500])
def test_dilate_mask_equals_iterated_three_wide_dilation(n):
    """n iterations of a [1, 1, 1] dilation with zero border (scipy's
    binary_dilation), restated naively, including both band ends and n
    larger than any run; n < 1 iterates until nothing changes."""
    from tricolour_amd import scan
    rs = np.random.RandomState(n)
    chans = np.arange(64, dtype=np.float64)
    for flags in (rs.uniform(size=64) < 0.05, np.eye(1, 64, 0, dtype=bool)[0], np.eye(1, 64, 63, dtype=bool)[0],
                  np.zeros(64, bool)):
        exp = flags.copy()
        for _ in range(n if n >= 1 else 64):
            exp = exp | np.concatenate([[False], exp[:-1]]) | np.concatenate([exp[1:], [False]])
        assert np.array_equal(scan.dilate_mask(chans, flags, str(n)), exp)


def test_dilate_mask_units():
    from tricolour_amd import scan
    chans = 1e9 + 2e5 * np.arange(32)
    flags = np.zeros(32, bool)
    flags[10] = True
    # 500 kHz / 200 kHz -> int(2.5) + 1 = 3 channels either side
    assert np.nonzero(scan.dilate_mask(chans, flags, "500kHz"))[0].tolist() == list(range(7, 14))
    assert np.array_equal(scan.dilate_mask(chans, flags, "0.5MHz"), scan.dilate_mask(chans, flags, "500000Hz"))
    with pytest.raises(ValueError, match="Unrecognised units"):
        scan.dilate_mask(chans, flags, "3Mhz")


def test_load_mask_rejects_wrong_dtype(tmp_path):
    from tricolour_amd import scan
    path = str(tmp_path / "bad.npy")
    arr = np.zeros((2, 8), dtype=[("mask", np.int32), ("chans", np.float64)])
    np.save(path, arr)
    with pytest.raises(ValueError, match="not a valid static mask"):
        scan.load_mask(path, "2")


def test_load_strategies(tmp_path):
    from tricolour_amd import scan
    path = tmp_path / "conf.yaml"
    path.write_text("""
# List of strategies to apply in order
strategies:
    -
        name: nan_dropouts_flag
        task: flag_nans_zeros
    -
        name: background_static_mask
        task: apply_static_mask
        kwargs:
            accumulation_mode: "or"
            uvrange: ""
    -
        name: background_flags
        task: sum_threshold
        kwargs:
            outlier_nsigma: 10
            windows_time: [1, 2, 4, 8]
            rho: 1.3
""")
    st = scan.load_strategies(str(path))
    assert [s["task"] for s in st] == ["flag_nans_zeros", "apply_static_mask", "sum_threshold"]
    assert st[1]["kwargs"] == {"accumulation_mode": "or", "uvrange": ""}
    assert st[2]["kwargs"]["windows_time"] == [1, 2, 4, 8] and st[2]["kwargs"]["rho"] == 1.3
    scan.check_strategies(st)
    bad = tmp_path / "bad.yaml"
    bad.write_text("something: else\n")
    with pytest.raises(ValueError):
        scan.load_strategies(str(bad))


def test_field_selection():
    from tricolour_amd import scan
    names = ["PKS1934", "J0408", "3C286"]
    assert scan.select_fields([], names) == {0: "PKS1934", 1: "J0408", 2: "3C286"}
    assert scan.select_fields(None, names) == {0: "PKS1934", 1: "J0408", 2: "3C286"}
    assert scan.select_fields(["J0408"], names) == {1: "J0408"}
    assert scan.select_fields(["PKS1934, 2"], names) == {0: "PKS1934", 2: "3C286"}
    assert scan.select_fields(["1", "3C286"], names) == {1: "J0408", 2: "3C286"}
    # an index past the table is dropped, as the reference does
    assert scan.select_fields(["0", "7"], names) == {0: "PKS1934"}
    with pytest.raises(ValueError, match="cannot be found"):
        scan.select_fields(["J0408,NOPE"], names)


def test_scan_selection():
    from tricolour_amd import scan
    assert sorted(scan.select_scans(None, [1, 2, 2, 5])) == [1, 2, 5]
    assert sorted(scan.select_scans([2, 5, 9], [1, 2, 2, 5])) == [2, 5]
    assert scan.select_scans([9], [1, 2]) == []


def _small_scan():
    rs = np.random.RandomState(0)
    a1, a2 = np.triu_indices(3, 0)
    shape = (a1.size, 8, 4)
    data = (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(np.complex64)
    return dict(data=data, flags=np.zeros(shape, bool), antenna1=a1.astype(np.int32),
                antenna2=a2.astype(np.int32), time=np.zeros(a1.size), chan_freq=np.arange(8.0) + 1e9,
                chan_width=np.ones(8))


def test_flag_scan_argument_checks():
    from tricolour_amd import scan
    s = _small_scan()
    args = (s["data"], s["flags"], s["antenna1"], s["antenna2"], s["time"], s["chan_freq"], s["chan_width"])
    st = [{"task": "flag_autos"}]
    with pytest.raises(ValueError, match="needs corr_type"):
        scan.flag_scan(*args, st, flagging_strategy="polarisation")
    with pytest.raises(ValueError, match="needs corr_type"):
        scan.flag_scan(*args, st, flagging_strategy="total_power")
    with pytest.raises(ValueError, match="Invalid flagging strategy"):
        scan.flag_scan(*args, st, flagging_strategy="stokes_i")
    with pytest.raises(ValueError) as err:
        scan.flag_scan(*args, [{"task": "flag_everything"}])
    assert err.value.args == ("Task '%s' does not name a valid task", "flag_everything")
    with pytest.raises(ValueError, match="has no 'task'"):
        scan.flag_scan(*args, [{"name": "x"}])
    with pytest.raises(ValueError, match="flags shape"):
        scan.flag_scan(s["data"], s["flags"][:, :4], *args[2:], st)
    with pytest.raises(ValueError, match="model shape"):
        scan.flag_scan(*args, st, model=s["data"][:-1])
    with pytest.raises(ValueError, match="one entry per row"):
        scan.flag_scan(s["data"], s["flags"], s["antenna1"][:-1], *args[3:], st)
    with pytest.raises(ValueError, match="one entry per channel"):
        scan.flag_scan(*args[:5], s["chan_freq"][:3], s["chan_width"], st)
    with pytest.raises(ValueError, match="form no Stokes parameter"):
        scan.flag_scan(*args, st, flagging_strategy="polarisation", corr_type=["XX", "XY", "YX", "LL"][:1] * 4)
    with pytest.raises(ValueError):
        scan.flag_scans([dict(DATA=s["data"], FLAG=s["flags"], FIELD_ID=0, SCAN_NUMBER=1)],
                        [{"task": "nope"}])
