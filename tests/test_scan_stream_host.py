"""Baseline-chunked scans on the host side: the chunk plan of
packing.scan_chunks against row_map, and flag_scan's / flag_scans' checks of
baseline_chunks, which run before the device is touched."""
import numpy as np
import pytest


def _scan(rs, na, ntime, autos=True, delete_frac=0.0, ndup=0, shuffle=False):
    a1, a2 = np.triu_indices(na, 0 if autos else 1)
    nbl = len(a1)
    ant1 = np.tile(a1, ntime).astype(np.int32)
    ant2 = np.tile(a2, ntime).astype(np.int32)
    tinv = np.repeat(np.arange(ntime), nbl).astype(np.int32)
    idx = np.nonzero(rs.uniform(size=ant1.size) >= delete_frac)[0]
    if ndup:
        idx = np.concatenate([idx, rs.choice(idx, ndup, replace=False)])
    if shuffle:
        idx = rs.permutation(idx)
    return ant1[idx], ant2[idx], tinv[idx]


SCANS = {
    # name: (antennas, dumps, autos, delete_frac, duplicates, shuffled rows)
    "plain": (6, 5, False, 0.0, 0, False),
    "autos": (6, 5, True, 0.0, 0, False),
    "missing_rows": (7, 6, True, 0.2, 0, False),
    "duplicated_cells": (5, 4, True, 0.0, 9, False),
    "not_time_ordered": (6, 7, True, 0.1, 4, True),
}


def _check_plan(ant1, ant2, tinv, n):
    from tricolour_amd import packing
    ubl = packing.unique_baselines(ant1, ant2)
    nbl = ubl.shape[0]
    ntime = int(tinv.max()) + 1
    row_bl, row_bl_pack, row_time = packing.row_map(ant1, ant2, ubl, tinv, ntime)
    chunks = list(packing.scan_chunks(ant1, ant2, ubl, tinv, ntime, n))
    assert len(chunks) == -(-nbl // n)
    seen = np.zeros(ant1.size, np.int64)
    for k, c in enumerate(chunks):
        assert (c.b0, c.b1) == (k * n, min((k + 1) * n, nbl))
        assert c.rows.dtype == np.int64 and c.pack.dtype == np.int64 and c.runs.dtype == np.int64
        assert np.all(np.diff(c.rows) > 0)                       # ascending, no repeats
        exp_rows = np.nonzero((row_bl >= c.b0) & (row_bl < c.b1))[0]
        assert np.array_equal(c.rows, exp_rows)
        seen[c.rows] += 1
        assert np.array_equal(c.bl, row_bl[c.rows] - c.b0) and np.all((c.bl >= 0) & (c.bl < c.b1 - c.b0))
        assert np.array_equal(c.time, row_time[c.rows])
        assert np.all(np.diff(c.pack) > 0)
        assert np.array_equal(c.pack_rows, c.rows[row_bl_pack[c.rows] >= 0])
        assert np.array_equal(row_bl_pack[c.pack_rows] - c.b0, c.bl[c.pack])
        # runs: maximal, and they concatenate back to the unpack list
        back = np.concatenate([np.arange(r0, r1) for r0, r1 in c.runs]) if len(c.runs) else np.zeros(0, np.int64)
        assert np.array_equal(back, c.rows)
        assert np.all(c.runs[:, 1] > c.runs[:, 0])
        assert np.all(c.runs[1:, 0] > c.runs[:-1, 1])
    assert np.all(seen == 1)                                     # every row in exactly one chunk
    return chunks


@pytest.mark.parametrize("name", sorted(SCANS))
@pytest.mark.parametrize("n", [1, 4, 7, 1000])
def test_scan_chunks_partition_the_scan(name, n):
    na, ntime, autos, delete_frac, ndup, shuffle = SCANS[name]
    rs = np.random.RandomState(na * 100 + ntime)
    ant1, ant2, tinv = _scan(rs, na, ntime, autos, delete_frac, ndup, shuffle)
    chunks = _check_plan(ant1, ant2, tinv, n)
    if n >= 1000:
        assert len(chunks) == 1 and chunks[0].rows.size == ant1.size


def test_scan_chunks_ragged_last_chunk_and_runs():
    from tricolour_amd import packing
    rs = np.random.RandomState(3)
    ant1, ant2, tinv = _scan(rs, 8, 3)                 # 36 baselines, time-major
    # rows of a dump in the order of unique_baselines (by antenna2, then antenna1)
    order = np.lexsort((ant1, ant2, tinv))
    ant1, ant2, tinv = ant1[order], ant2[order], tinv[order]
    chunks = _check_plan(ant1, ant2, tinv, 16)
    assert [c.b1 - c.b0 for c in chunks] == [16, 16, 4]
    # one run of N rows per dump
    assert [len(c.runs) for c in chunks] == [3, 3, 3]
    assert all(np.all(c.runs[:, 1] - c.runs[:, 0] == c.b1 - c.b0) for c in chunks)
    # duplicates of a cell: the LAST row of the cell is the one packed
    ant1 = np.concatenate([ant1, ant1[:2]])
    ant2 = np.concatenate([ant2, ant2[:2]])
    tinv = np.concatenate([tinv, tinv[:2]])
    chunks = _check_plan(ant1, ant2, tinv, 16)
    assert not np.isin([0, 1], chunks[0].pack_rows).any()
    assert np.isin([ant1.size - 2, ant1.size - 1], chunks[0].pack_rows).all()
    with pytest.raises(ValueError):
        list(packing.scan_chunks(ant1, ant2, packing.unique_baselines(ant1, ant2), tinv, 3, 0))


def _small_scan():
    rs = np.random.RandomState(0)
    a1, a2 = np.triu_indices(3, 0)
    shape = (a1.size, 8, 4)
    data = (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(np.complex64)
    return (data, np.zeros(shape, bool), a1.astype(np.int32), a2.astype(np.int32), np.zeros(a1.size),
            np.arange(8.0) + 1e9, np.ones(8))


@pytest.mark.parametrize("bad", [0, -1, -16, 2.0, 1.5, "4", True, np.float64(3.0)])
def test_flag_scan_rejects_bad_baseline_chunks(bad):
    from tricolour_amd import scan
    with pytest.raises(ValueError, match="baseline_chunks"):
        scan.flag_scan(*_small_scan(), [{"task": "flag_autos"}], baseline_chunks=bad)
    with pytest.raises(ValueError, match="baseline_chunks"):
        scan.flag_scans([], [{"task": "flag_autos"}], baseline_chunks=bad)
