"""Log-binned amplitude histograms of the kept and the flagged samples (tricolour_amd.quality.window_histograms,
tri_amplitude_histogram) against a host restatement.

restate() is numpy per the definition: the canonical amplitude float32(sqrt(float64(re)^2 + float64(im)^2)) (|x| for
float32), the slot rule on its bit pattern, and np.add.at.  Counts are integers, so every comparison is exact equality:
there is no tolerance anywhere in the device tests.  The statistics derived on the host (quantile, noise_sigma,
tail_excess) are held to hand-made counts and to Rayleigh samples."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

from tricolour_amd import _lib, flagging, quality
from tricolour_amd.quality import AmplitudeBins, AmplitudeHistograms

HPP = os.path.join(ROOT, "tricolour_amd", "csrc", "steps", "hist", "kernels_hist.hpp")


def header_constants():
    """The HIST_* constants of the kernel header, evaluated."""
    out = {}
    with open(HPP) as fh:
        for name, expr in re.findall(r"^#define[ \t]+(HIST_\w+)[ \t]+(.+?)[ \t]*(?://.*)?$", fh.read(), re.M):
            out[name] = int(eval(expr, {"__builtins__": {}}, dict(out)))
    return out


H = header_constants()
V, SPAN, R, NT, CPL = H["HIST_V"], H["HIST_SPAN"], H["HIST_ROWS"], H["HIST_NT"], H["HIST_CPL"]

BIN_SETS = [(-24, 24, 3), (-126, 128, 3), (0, 1, 0), (-10, 12, 5)]


# ---- the restatement ----

def ref_slots(vis, emin, emax, sub_bits):
    """The slot of every sample by the definition, written out here (not through AmplitudeBins)."""
    vis = np.asarray(vis)
    nb = (emax - emin) << sub_bits
    if np.iscomplexobj(vis):
        re_, im_ = vis.real.astype(np.float64), vis.imag.astype(np.float64)
        finite = np.isfinite(re_) & np.isfinite(im_)
        with np.errstate(invalid="ignore", over="ignore"):
            a = np.sqrt(re_ ** 2 + im_ ** 2).astype(np.float32)
    else:
        assert vis.dtype == np.float32
        finite = np.isfinite(vis)
        a = np.abs(vis)
    u = np.ascontiguousarray(a).view(np.uint32).astype(np.int64)
    k = (u >> (23 - sub_bits)) - ((emin + 127) << sub_bits)
    slot = np.where(k < 0, 0, np.where(k >= nb, nb + 1, k + 1))
    return np.where(finite, slot, nb + 2)


def restate(vis, flags, bins, freq_chunks):
    """(hist_bl, hist_chunk, chunk ends) of the definition."""
    nbl, ncorr, ntime, nchan = vis.shape
    ends = np.linspace(0, nchan, freq_chunks + 1).astype(np.int64)
    slot = ref_slots(vis, bins.emin, bins.emax, bins.sub_bits)
    pop = (np.asarray(flags) != 0).astype(np.int64)
    b, c, _t, f = np.meshgrid(np.arange(nbl), np.arange(ncorr), np.arange(ntime), np.arange(nchan), indexing="ij")
    chunk_of = np.searchsorted(ends, f, "right") - 1
    hist_bl = np.zeros((nbl, ncorr, 2, bins.slots), np.int64)
    hist_chunk = np.zeros((ncorr, freq_chunks, 2, bins.slots), np.int64)
    np.add.at(hist_bl, (b, c, pop, slot), 1)
    np.add.at(hist_chunk, (c, chunk_of, pop, slot), 1)
    return hist_bl, hist_chunk, ends


def same_counts(got, want_bl, want_chunk):
    assert got.bl.dtype == np.int64 and got.chunk.dtype == np.int64
    assert got.bl.shape == want_bl.shape and got.chunk.shape == want_chunk.shape, (got.bl.shape, got.chunk.shape)
    assert np.array_equal(got.bl, want_bl), int((got.bl != want_bl).sum())
    assert np.array_equal(got.chunk, want_chunk), int((got.chunk != want_chunk).sum())


def mixed(shape, seed, dtype="c64"):
    """Magnitudes over 80 octaves, both signs, with zeros, subnormals and huge values among them."""
    rs = np.random.RandomState(seed)

    def part():
        x = (np.exp2(rs.uniform(-40.0, 40.0, shape)) * rs.choice([-1.0, 1.0], shape)).astype(np.float32)
        kind = rs.randint(0, 40, shape)
        x[kind == 0] = 0.0
        x[kind == 1] = np.float32(1e-41)                         # subnormal
        x[kind == 2] = np.finfo(np.float32).max
        x[kind == 3] = np.float32(1.0)
        return x
    if dtype == "f32":
        return part()
    return (part() + 1j * part()).astype(np.complex64)


def random_flags(shape, seed, frac=0.3):
    return np.random.RandomState(seed).random_sample(shape) < frac


def plant_nonfinite(vis, freq_chunks):
    """NaN / Inf at the first and last column, either side of a load's, a chunk's and a span's edge, in the rows either
    side of a band's edge."""
    ntime, nchan = vis.shape[2:]
    ends = np.linspace(0, nchan, freq_chunks + 1).astype(np.int64).tolist()
    cols = {0, nchan - 1, V - 1, V, SPAN - 1, SPAN}
    for e in ends:
        cols.update((e - 1, e, e + SPAN - 1, e + SPAN))
    cols = sorted(c for c in cols if 0 <= c < nchan)[:64]
    rows = sorted(t for t in {0, R - 1, R, ntime - 1} if 0 <= t < ntime)
    bad = [np.nan, np.inf, -np.inf]
    for k, c in enumerate(cols):
        t = rows[k % len(rows)]
        vis[k % vis.shape[0], k % vis.shape[1], t, c] = bad[k % 3] if vis.dtype == np.float32 else \
            (complex(bad[k % 3], 1.0) if k % 2 else complex(1.0, bad[k % 3]))
    return vis


# ---- CPU ----

def test_abi_declares_and_exports_the_entry_points():
    hdr = open(_lib.HEADER).read()
    for name in ("tri_histogram_slots", "tri_amplitude_histogram"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().tri_version() >= 108
    assert HPP in _lib.DEPENDS
    assert re.search(r"^#define\s+TRI_MAX_HIST_BINS\s+%d\b" % _lib.TRI_MAX_HIST_BINS, hdr, re.M)
    assert _lib.TRI_MAX_HIST_BINS == 2048
    # a band of rows times a span of channels stays far below what a 32-bit counter holds
    assert R * SPAN < 1 << 32 and SPAN == NT * V
    # the Python layer batches baselines under the header's launch limit
    assert quality._hist_cap(1, 3 * R) == H["HIST_MAX_GRID_X"] // 3 and quality._hist_cap(4, 3 * R + 1) == H["HIST_MAX_GRID_X"] // 4 // 4
    assert H["HIST_MAX_GRID_X"] * NT < 1 << 32 and quality._hist_cap(1 << 30, 1 << 30) == 1


def test_histogram_slots():
    slots = _lib.lib().tri_histogram_slots
    assert slots(-24, 24, 3) == 48 * 8 + 3 and slots(0, 1, 0) == 4 and slots(-10, 12, 5) == 22 * 32 + 3
    assert slots(-126, 128, 3) == 254 * 8 + 3 and slots(-126, 128, 3) - 3 <= _lib.TRI_MAX_HIST_BINS
    assert slots(-64, 0, 5) == 2048 + 3                                                # exactly the most bins
    for bad in ((-127, 0, 0), (0, 129, 0), (3, 3, 0), (4, 3, 0), (0, 1, -1), (0, 1, 6), (-126, 128, 4), (-64, 1, 5)):
        assert slots(*bad) == 0, bad
        with pytest.raises(ValueError):
            AmplitudeBins(*bad)
    for ok in BIN_SETS:
        b = AmplitudeBins(*ok)
        assert b.slots == slots(*ok) == b.nb + 3 and b.edges().shape == (b.nb + 1,) and b.edges().dtype == np.float64
    for wrong in (1.5, "3", None, True):
        with pytest.raises(ValueError):
            AmplitudeBins(sub_bits=wrong)
    assert AmplitudeBins() == AmplitudeBins(-24, 24, 3) and AmplitudeBins() != AmplitudeBins(-24, 24, 2)


def test_abi_rejects_bad_arguments_without_a_launch():
    lib = _lib.lib()
    buf = (C.c_uint8 * (8 * 4096))()
    base = C.addressof(buf)
    v, f, hb, hc = (base + 4096 * i for i in range(4))
    good_ends = [0, 4, 8]

    def call(vis=v, dtype=_lib.TRI_VIS_C64, flags=f, n_bl=2, n_corr=2, ntime=4, nchan=8, ends=good_ends, n_ends=None,
             bins=(0, 1, 0), hb=hb, hc=hc, acc=0):
        arr = None if ends is None else (C.c_int64 * len(ends))(*ends)
        return lib.tri_amplitude_histogram(vis, dtype, flags, n_bl, n_corr, ntime, nchan, arr,
                                           (len(ends) if ends is not None else 3) if n_ends is None else n_ends,
                                           bins[0], bins[1], bins[2], hb, hc, acc, None)
    for name in ("vis", "flags", "ends", "hb", "hc"):
        assert call(**{name: None}) == _lib.TRI_EINVAL, name
    for name in ("n_bl", "n_corr", "ntime", "nchan"):
        assert call(**{name: -1}) == _lib.TRI_EINVAL, name
    for dt in (_lib.TRI_VIS_C128, _lib.TRI_VIS_F64, 17, -1):
        assert call(dtype=dt) == _lib.TRI_EINVAL, dt
    for bins in ((-127, 0, 0), (0, 129, 0), (3, 3, 0), (0, 1, 6), (0, 1, -1), (-126, 128, 4)):
        assert call(bins=bins) == _lib.TRI_EINVAL, bins
    for ends in ([1, 4, 8], [0, 4, 7], [0, 4, 9], [0, 5, 4, 8], [0, -1, 8], [8]):
        assert call(ends=ends) == _lib.TRI_EINVAL, ends
    assert call(n_ends=1) == _lib.TRI_EINVAL and call(n_ends=0) == _lib.TRI_EINVAL
    # outputs over an input, over each other (256 bytes each; vis holds 1024, flags 128)
    for kw in (dict(hb=v + 8), dict(hb=f), dict(hc=v + 1016), dict(hc=f + 127), dict(hc=hb), dict(hc=hb + 248), dict(hb=hc - 8)):
        assert call(**kw) == _lib.TRI_EINVAL, kw
    assert b"overlap" in lib.tri_last_error()
    # beyond the launch geometry
    for kw in (dict(ntime=1 << 31), dict(n_bl=1 << 31), dict(n_corr=1 << 31), dict(n_bl=1 << 20, n_corr=1 << 20),
               dict(n_bl=1 << 24, n_corr=1), dict(n_bl=1 << 23, n_corr=1, ntime=2 * R),
               dict(nchan=1 << 31, ends=[0, 1 << 31]), dict(nchan=65535 * SPAN + 1, ends=[0, 65535 * SPAN + 1])):
        assert call(**kw) == _lib.TRI_EUNSUPPORTED, kw
    # an empty shape that leaves nothing to write: no launch, no device
    assert call(n_corr=0) == _lib.TRI_OK
    assert call(n_bl=0, acc=1) == _lib.TRI_OK
    # argument errors win over the empty shape
    assert call(n_bl=0, vis=None) == _lib.TRI_EINVAL and call(n_corr=0, dtype=9) == _lib.TRI_EINVAL
    assert call(n_corr=0, bins=(0, 0, 0)) == _lib.TRI_EINVAL and call(n_bl=0, ends=[0, 9]) == _lib.TRI_EINVAL


def _planted(bins):
    """float32 amplitudes that sit on and beside everything the slot rule distinguishes."""
    edges = bins.edges()
    inside = edges[edges <= float(np.finfo(np.float32).max)].astype(np.float32)
    assert np.array_equal(inside.astype(np.float64), edges[:inside.size])            # every such edge is a float32
    below = np.nextafter(inside, np.float32(0))
    above = np.nextafter(inside, np.float32(np.inf))
    tiny = np.array([0.0, 1e-45, 1e-41, 1.1754942e-38, 1.17549435e-38, 2.0 ** bins.emin if bins.emin > -127 else 0.0],
                    np.float32)
    top = np.array([np.finfo(np.float32).max, 3e38, 1.0, 1.5, 2.0, 0.75], np.float32)
    return np.concatenate([inside, below, above, tiny, top])


@pytest.mark.parametrize("b", BIN_SETS + [(-126, -120, 5), (120, 128, 5), (-3, 2, 1)], ids=str)
def test_slot_of_is_a_search_in_the_edges(b):
    bins = AmplitudeBins(*b)
    edges = bins.edges()
    assert (np.diff(edges) > 0).all() and edges[0] == 2.0 ** bins.emin and edges[-1] == 2.0 ** bins.emax
    rs = np.random.RandomState(7)
    with np.errstate(over="ignore"):
        a = np.concatenate([np.exp2(rs.uniform(-150.0, 128.0, 200000)).astype(np.float32),
                            rs.random_sample(1000).astype(np.float32), _planted(bins)])
    a = a[np.isfinite(a)]
    slot = bins.slot_of(a)
    assert slot.dtype == np.int64 and np.array_equal(slot, np.searchsorted(edges, a.astype(np.float64), "right"))
    assert np.array_equal(slot, ref_slots(a, *b))
    assert np.array_equal(bins.slot_of(-a), slot)                                      # |x|
    # planted: zero and a subnormal underflow, an edge opens its bin, the float below it closes the one before
    assert bins.slot_of(np.float32([0.0, 1e-41])).tolist() == [0, 0]
    assert bins.slot_of(np.float32([2.0 ** bins.emin])).tolist() == [1]
    lo = np.nextafter(np.float32(2.0 ** bins.emin), np.float32(0))
    assert bins.slot_of(np.array([lo], np.float32)).tolist() == [0]
    if bins.emax < 128:
        top = np.float32(2.0 ** bins.emax)
        assert bins.slot_of(np.array([np.nextafter(top, np.float32(0)), top], np.float32)).tolist() == [bins.nb, bins.nb + 1]
    else:
        assert bins.slot_of(np.float32([np.finfo(np.float32).max])).tolist() == [bins.nb]
    # non-finite amplitudes and parts; finite parts whose amplitude rounds to +Inf overflow
    assert bins.slot_of(np.float32([np.nan, np.inf, -np.inf])).tolist() == [bins.nb + 2] * 3
    big = np.finfo(np.float32).max
    z = np.array([complex(big, big), complex(np.nan, 1), complex(1, np.inf), complex(-np.inf, np.nan), 0j], np.complex64)
    assert bins.slot_of(z).tolist() == [bins.nb + 1, bins.nb + 2, bins.nb + 2, bins.nb + 2, 0]
    assert np.array_equal(bins.slot_of(z), ref_slots(z, *b))
    # complex samples: the slot of the canonical amplitude
    zz = mixed((4000,), 3)
    with np.errstate(over="ignore"):
        amp = np.sqrt(zz.real.astype(np.float64) ** 2 + zz.imag.astype(np.float64) ** 2).astype(np.float32)
    fin = np.isfinite(amp)
    assert np.array_equal(bins.slot_of(zz)[fin], bins.slot_of(amp[fin])) and (bins.slot_of(zz)[~fin] == bins.nb + 1).all()


def _hand_made(counts, bins):
    """AmplitudeHistograms with one chunk cell whose kept population holds ``counts`` (slots 0 .. nb + 1)."""
    chunk = np.zeros((1, 1, 2, bins.slots), np.int64)
    chunk[0, 0, 0, :len(counts)] = counts
    return AmplitudeHistograms(np.zeros((0, 1, 2, bins.slots), np.int64), chunk, bins, [0, 1], (0, 1, 1, 1))


def test_quantile_on_hand_made_counts():
    bins = AmplitudeBins(0, 2, 1)                                  # edges 1, 1.5, 2, 3, 4: slots 0 | 1 2 3 4 | 5 | 6
    assert bins.edges().tolist() == [1.0, 1.5, 2.0, 3.0, 4.0]
    h = _hand_made([0, 4, 0, 4, 0, 0], bins)
    qt = lambda hh, q: float(hh.quantile("chunk", q)[0, 0])
    assert qt(h, 0.25) == 1.25 and qt(h, 0.5) == 1.5               # rank 4 is reached in slot 1: its upper edge
    assert qt(h, 0.75) == 2.5 and qt(h, 1.0) == 3.0                # the empty slot 2 is skipped
    assert qt(h, 0.0) == 1.0                                       # the first non-empty slot, not the empty underflow
    assert h.counts("chunk").shape == (1, 1, bins.nb + 2) and h.counts("chunk", "flagged").sum() == 0
    u = _hand_made([6, 2, 0, 0, 0, 2], bins)
    assert qt(u, 0.5) == 0.0 and qt(u, 0.6) == 0.0 and qt(u, 0.7) == 1.25 and qt(u, 0.9) == np.inf and qt(u, 1.0) == np.inf
    empty = _hand_made([0] * 6, bins)
    assert np.isnan(qt(empty, 0.5)) and np.isnan(empty.noise_sigma("chunk")[0, 0]) and np.isnan(empty.tail_excess("chunk")[0, 0])
    # the non-finite slot takes no part
    nf = _hand_made([0, 4, 0, 4, 0, 0], bins)
    nf.chunk[0, 0, 0, bins.nb + 2] = 1000
    assert qt(nf, 0.5) == 1.5
    # the flagged population on request
    nf.chunk[0, 0, 1, 3] = 2
    assert float(nf.quantile("chunk", 0.5, population=1)[0, 0]) == 2.5
    assert float(h.noise_sigma("chunk")[0, 0]) == 1.5 / np.sqrt(2.0 * np.log(2.0))
    for bad in (dict(axis="time", q=0.5), dict(axis="chunk", q=1.5), dict(axis="bl", q=0.5, population=2)):
        with pytest.raises(ValueError):
            h.quantile(**bad)
    assert h.quantile("bl", 0.5).shape == (0, 1)


def _numpy_histograms(a, bins):
    chunk = np.zeros((1, 1, 2, bins.slots), np.int64)
    np.add.at(chunk[0, 0, 0], bins.slot_of(a), 1)
    return AmplitudeHistograms(np.zeros((0, 1, 2, bins.slots), np.int64), chunk, bins, [0, 1], (0, 1, 1, a.size))


@pytest.mark.parametrize("seed", range(5))
def test_statistics_of_rayleigh_samples(seed):
    """Unit Rayleigh amplitudes: the median gives sigma to 1 %, the tail above 4 sigma holds what the law says to a
    factor of 2 (67 samples are expected above the edge 4.0, 8 above the edge 4.5 that a sigma just over 1 selects), and
    0.5 % of the samples moved up by 8 sigma show as an excess above 20."""
    rs = np.random.RandomState(seed)
    n = 200000
    a = np.hypot(rs.standard_normal(n), rs.standard_normal(n)).astype(np.float32)
    bins = AmplitudeBins(sub_bits=3)
    h = _numpy_histograms(a, bins)
    sigma, excess = float(h.noise_sigma("chunk")[0, 0]), float(h.tail_excess("chunk", 4.0)[0, 0])
    print("seed %d: sigma %.5f, tail_excess(4) %.3f" % (seed, sigma, excess))
    assert int(h.counts("chunk").sum()) == n
    assert abs(sigma - 1.0) < 0.01
    assert 0.5 < excess < 2.0
    dirty = a.copy()
    dirty[rs.choice(n, n // 200, replace=False)] += np.float32(8.0)
    hd = _numpy_histograms(dirty, bins)
    sigma_d, excess_d = float(hd.noise_sigma("chunk")[0, 0]), float(hd.tail_excess("chunk", 4.0)[0, 0])
    print("contaminated: sigma %.5f, tail_excess(4) %.3f" % (sigma_d, excess_d))
    assert excess_d > 20.0 and abs(sigma_d - 1.0) < 0.02
    lines = quality.summarise_histograms(hd, h)
    assert lines[3] == "Per correlation, kept samples over all chunks:" and "tail excess" in lines[4]


def test_python_layer_checks_without_a_device():
    vis, flags = np.zeros((0, 2, 3, 8), np.complex64), np.zeros((0, 2, 3, 8), bool)
    h = quality.window_histograms(vis, flags, AmplitudeBins(0, 1, 0), 2)
    assert h.bl.shape == (0, 2, 2, 4) and h.chunk.shape == (2, 2, 2, 4) and h.chunk.dtype == np.int64 and not h.chunk.any()
    assert h.shape == (0, 2, 3, 8) and h.chunk_ends.tolist() == [0, 4, 8] and h.bins == AmplitudeBins(0, 1, 0)
    prev = AmplitudeHistograms(np.ones((3, 2, 2, 4), np.int64), np.full((2, 2, 2, 4), 5, np.int64), AmplitudeBins(0, 1, 0),
                               [0, 4, 8], (3, 2, 3, 8))
    more = quality.window_histograms(vis, flags, AmplitudeBins(0, 1, 0), 2, accumulate_into=prev)
    assert more.shape == (3, 2, 3, 8) and np.array_equal(more.bl, prev.bl) and np.array_equal(more.chunk, prev.chunk)
    for kw in (dict(bins=AmplitudeBins(0, 2, 0)), dict(freq_chunks=4), dict(vis=np.zeros((0, 2, 3, 9), np.complex64)),
               dict(vis=np.zeros((0, 1, 3, 8), np.complex64))):
        v = kw.pop("vis", vis)
        args = dict(bins=AmplitudeBins(0, 1, 0), freq_chunks=2)
        args.update(kw)
        with pytest.raises(ValueError):
            quality.window_histograms(v, np.zeros(v.shape, bool), accumulate_into=prev, **args)
    for kw in (dict(bins=(0, 1, 0)), dict(freq_chunks=0), dict(freq_chunks=2.5), dict(accumulate_into=object())):
        with pytest.raises(ValueError):
            quality.window_histograms(vis, flags, **kw)
    with pytest.raises(ValueError):
        quality.window_histograms(vis, np.zeros((0, 2, 3, 7), bool))
    with pytest.raises(ValueError):
        quality.window_histograms(np.zeros((2, 3, 8), np.complex64), np.zeros((2, 3, 8), bool))


def test_scan_quality_keeps_its_plain_form():
    q = quality.ScanQuality()
    assert (q.original, q.final, q.ubl, q.chan_freq, q.times) == (None,) * 5
    assert q.histograms is None and q.original_histograms is None and q.final_histograms is None
    qh = quality.ScanQuality(histograms=AmplitudeBins(-10, 12, 5), freq_chunks=3)
    assert (qh.original, qh.final, qh.ubl, qh.chan_freq, qh.times) == (None,) * 5
    assert qh.histograms == AmplitudeBins(-10, 12, 5) and qh.freq_chunks == 3
    for bad in (dict(histograms=(0, 1, 0)), dict(histograms=True), dict(freq_chunks=0)):
        with pytest.raises(ValueError):
            quality.ScanQuality(**bad)
    from tricolour_amd import scan
    with pytest.raises(ValueError):
        scan.flag_scans([], [{"task": "flag_autos"}], histograms=AmplitudeBins())
    with pytest.raises(ValueError):
        scan.flag_scans([], [{"task": "flag_autos"}], quality=[], histograms="yes")
    code = ("import sys; from tricolour_amd.quality import AmplitudeBins, AmplitudeHistograms, window_histograms, "
            "summarise_histograms, ScanQuality; AmplitudeBins().slot_of([1.0]); "
            "assert 'torch' not in sys.modules, 'torch was imported'")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True, timeout=120)


# ---- GPU ----

# (shape, freq_chunks): one sample; either side of the load width and of a block's channel span, as one chunk and as
# ten; either side of the row band; unaligned chunk ends; more chunks than channels, and than one launch holds
CASES = [((1, 1, 1, 1), 1)]
CASES += [((2, 1, 3, c), k) for c in (V - 1, V, V + 1, SPAN - 1, SPAN, SPAN + 1) for k in (1, 10)]
CASES += [((1, 2, R - 1, 37), 3), ((1, 2, R + 1, 37), 3), ((2, 2, 5, 37), 3), ((2, 2, 5, 37), 1), ((2, 1, 3, 37), 50),
          ((1, 1, 2, 3 * SPAN + 8), 3), ((1, 2, 2, 72), CPL + 5), ((3, 2, R + 3, 2 * SPAN + V), 2)]


def _case_id(case):
    return "x".join(map(str, case[0])) + "-%d" % case[1]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_gpu_counts_equal_the_restatement(gpu, case, dtype):
    shape, freq_chunks = case
    vis = plant_nonfinite(mixed(shape, sum(shape) + freq_chunks, dtype), freq_chunks)
    if dtype == "f32":
        assert (vis[np.isfinite(vis)] < 0).any() or vis.size < 4
    rnd = random_flags(shape, 11 + sum(shape))
    nbl, ncorr, ntime, nchan = shape
    kept_vis, kept_flags = vis.copy(), None
    for b in BIN_SETS:
        bins = AmplitudeBins(*b)
        for flags in (rnd, rnd.astype(np.uint8) * 3, np.ones(shape, bool), np.zeros(shape, np.uint8)):
            kept_flags = flags.copy()
            got = quality.window_histograms(vis, flags, bins, freq_chunks)
            want_bl, want_chunk, ends = restate(vis, flags, bins, freq_chunks)
            assert isinstance(got, AmplitudeHistograms) and got.shape == shape and got.bins == bins
            assert np.array_equal(got.chunk_ends, ends) and np.array_equal(ends, flagging._chunk_ends(nchan, freq_chunks)[0])
            same_counts(got, want_bl, want_chunk)
            # every sample is counted once
            assert (got.bl.sum(axis=(2, 3)) == ntime * nchan).all()
            assert np.array_equal(got.chunk.sum(axis=(2, 3)), np.broadcast_to(nbl * ntime * np.diff(ends), (ncorr, freq_chunks)))
            if flags.all():
                assert not got.bl[:, :, 0].any() and not got.chunk[:, :, 0].any()
            if not flags.any():
                assert not got.bl[:, :, 1].any() and not got.chunk[:, :, 1].any()
            # inputs untouched
            assert np.array_equal(vis.view(np.uint32), kept_vis.view(np.uint32)) and np.array_equal(flags, kept_flags)


@pytest.mark.gpu
@pytest.mark.parametrize("b", BIN_SETS, ids=str)
def test_gpu_amplitudes_on_bin_edges(gpu, b):
    """Every edge that is a float32, the float below and the float above it, as float32 amplitudes of either sign and as
    complex samples along either axis (whose canonical amplitude is the edge itself)."""
    bins = AmplitudeBins(*b)
    a = _planted(bins)
    a = np.concatenate([a, np.zeros(-a.size % 12, np.float32)]).reshape(1, 2, 6, -1)
    a[0, 1] *= np.float32(-1)
    flags = random_flags(a.shape, 5)
    for vis in (a, a.astype(np.complex64), (1j * a).astype(np.complex64)):
        got = quality.window_histograms(vis, flags, bins, 3)
        same_counts(got, *restate(vis, flags, bins, 3)[:2])
        # and the slots are those of a search in the edges
        slot = np.searchsorted(bins.edges(), np.abs(a).astype(np.float64), "right")
        want = np.zeros((2, 2, bins.slots), np.int64)
        np.add.at(want, (np.arange(2)[None, :, None, None], flags.astype(np.int64), slot), 1)
        assert np.array_equal(got.bl[0], want)


@pytest.mark.gpu
def test_gpu_one_bin_takes_every_sample(gpu):
    """Every sample equal: one counter holds 90 000, far above what 16 bits hold, and every lane of every wave adds to
    the same LDS address."""
    shape = (1, 1, 300, 300)
    bins = AmplitudeBins()
    for vis in (np.full(shape, 3 + 4j, np.complex64), np.full(shape, -5.0, np.float32)):
        for flags in (np.zeros(shape, bool), np.ones(shape, bool)):
            got = quality.window_histograms(vis, flags, bins, 1)
            slot = int(bins.slot_of(np.float32([5.0]))[0])
            want = np.zeros((1, 1, 2, bins.slots), np.int64)
            want[0, 0, int(flags.any()), slot] = 300 * 300
            same_counts(got, want, want)
            same_counts(got, *restate(vis, flags, bins, 1)[:2])


@pytest.mark.gpu
def test_gpu_outputs_are_written_whole_and_nothing_beside_them(gpu):
    """Through the ABI, both outputs inside guard bands and pre-filled with garbage: accumulate = 0 gives the
    restatement's counts, accumulate = 1 continues hist_chunk and writes hist_bl fresh, no byte either side changes;
    a base that is not 16-byte aligned takes the scalar route to the same counts."""
    import torch
    from scratch_poison import Output
    lib = _lib.lib()
    shape = (3, 2, R + 2, 2 * SPAN)
    nbl, ncorr, ntime, nchan = shape
    bins, freq_chunks = AmplitudeBins(-10, 12, 5), 5
    vis, flags = plant_nonfinite(mixed(shape, 61), freq_chunks), random_flags(shape, 62)
    want_bl, want_chunk, ends = restate(vis, flags, bins, freq_chunks)
    c_ends = (C.c_int64 * len(ends))(*[int(e) for e in ends])
    n = int(np.prod(shape))
    stream = torch.cuda.current_stream().cuda_stream
    for offset, vec in ((0, "true"), (1, "false")):
        v = torch.empty(n + 4, dtype=torch.complex64, device="cuda")[offset:offset + n].view(shape)
        f = torch.empty(n + 4, dtype=torch.uint8, device="cuda")[offset:offset + n].view(shape)
        v.copy_(torch.from_numpy(vis))
        f.copy_(torch.from_numpy(flags.view(np.uint8)))
        hb = Output((nbl, ncorr, 2, bins.slots), torch.int64, "cuda")
        hc = Output((ncorr, freq_chunks, 2, bins.slots), torch.int64, "cuda")

        def call(acc):
            _lib.check(lib.tri_amplitude_histogram(v.data_ptr(), _lib.TRI_VIS_C64, f.data_ptr(), nbl, ncorr, ntime, nchan,
                                                   c_ends, len(ends), bins.emin, bins.emax, bins.sub_bits, hb.ptr, hc.ptr,
                                                   acc, stream))
        _lib.kernel_log_begin()
        try:
            call(0)
        finally:
            log = _lib.kernel_log_end()
        assert set(log) == {"k_hist_fill<0, %s>" % vec} and log["k_hist_fill<0, %s>" % vec] == 1, log
        assert np.array_equal(hb.host(), want_bl) and np.array_equal(hc.host(), want_chunk)
        call(1)
        assert np.array_equal(hb.host(), want_bl) and np.array_equal(hc.host(), 2 * want_chunk)
        call(0)
        assert np.array_equal(hb.host(), want_bl) and np.array_equal(hc.host(), want_chunk)
        assert hb.damaged() == 0 and hc.damaged() == 0
        assert np.array_equal(v.cpu().numpy().view(np.uint32), vis.view(np.uint32)) and np.array_equal(f.cpu().numpy(), flags.view(np.uint8))
    # an empty call writes zeros, or leaves the accumulated cells alone, without a launch
    _lib.kernel_log_begin()
    try:
        for acc in (1, 0):
            _lib.check(lib.tri_amplitude_histogram(v.data_ptr(), _lib.TRI_VIS_C64, f.data_ptr(), 0, ncorr, ntime, nchan,
                                                   c_ends, len(ends), bins.emin, bins.emax, bins.sub_bits, hb.ptr, hc.ptr,
                                                   acc, stream))
            assert bool(hc.host().any()) == bool(acc)
    finally:
        assert not _lib.kernel_log_end()
    assert hb.damaged() == 0 and hc.damaged() == 0


@pytest.mark.gpu
def test_gpu_batches_halves_and_tensors_give_the_same_counts(gpu):
    import torch
    shape = (5, 2, R + 5, 300)
    bins = AmplitudeBins()
    vis, flags = plant_nonfinite(mixed(shape, 41), 10), random_flags(shape, 42)
    one = quality.window_histograms(vis, flags)
    assert one.bins == bins and one.chunk.shape == (2, 10, 2, bins.slots)
    same_counts(one, *restate(vis, flags, bins, 10)[:2])
    same_counts(quality.window_histograms(vis, flags), one.bl, one.chunk)
    _lib.kernel_log_begin()
    try:
        each = quality.window_histograms(vis, flags, _max_baselines=1)
    finally:
        log = _lib.kernel_log_end()
    assert sum(log.values()) == 5 and all(k.startswith("k_hist_fill<0, ") for k in log), log
    same_counts(each, one.bl, one.chunk)
    same_counts(quality.window_histograms(vis, flags, _max_baselines=2), one.bl, one.chunk)
    head = quality.window_histograms(vis[:3], flags[:3])
    kept = head.chunk.copy()
    both = quality.window_histograms(vis[3:], flags[3:], accumulate_into=head)
    assert both.shape == shape and np.array_equal(head.chunk, kept)
    same_counts(both, one.bl, one.chunk)
    with pytest.raises(ValueError):
        quality.window_histograms(vis[3:], flags[3:], bins, 9, accumulate_into=head)
    # ROCm tensors, bool and uint8 flags
    v, f = torch.from_numpy(vis).cuda(), torch.from_numpy(flags).cuda()
    same_counts(quality.window_histograms(v, f), one.bl, one.chunk)
    same_counts(quality.window_histograms(v, f.view(torch.uint8) * 7), one.bl, one.chunk)
    assert np.array_equal(v.cpu().numpy().view(np.uint32), vis.view(np.uint32)) and np.array_equal(f.cpu().numpy(), flags)
    # the derived values of real counts: finite where samples were kept
    assert np.isfinite(one.noise_sigma("bl")).all() and one.quantile("chunk", 0.5).shape == (2, 10)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["standard", "total_power"])
def test_gpu_flag_scan_fills_the_histograms_of_the_packed_windows(gpu, mode):
    from tricolour_amd import packing, scan
    from tricolour_amd.strategies import apply_strategies
    from test_quality import quality_scan, same_bits
    data, flags, ant1, ant2, tm, freq, width = quality_scan(51)
    strategies = [{"task": "flag_autos"},
                  {"task": "sum_threshold", "kwargs": dict(num_major_iterations=1, background_iterations=1)}]
    kw = dict(flagging_strategy=mode, corr_type=[9, 12])
    bins = AmplitudeBins(-10, 12, 5)
    plain_q = quality.ScanQuality()
    _lib.kernel_log_begin()
    try:
        plain = scan.flag_scan(data, flags, ant1, ant2, tm, freq, width, strategies, quality=plain_q, **kw)
    finally:
        log = _lib.kernel_log_end()
    assert not [k for k in log if k.startswith("k_hist")] and [k for k in log if k.startswith("k_quality")], log
    assert plain_q.original_histograms is None and plain_q.final_histograms is None
    q = quality.ScanQuality(histograms=bins, freq_chunks=3)
    _lib.kernel_log_begin()
    try:
        whole = scan.flag_scan(data, flags, ant1, ant2, tm, freq, width, strategies, quality=q, **kw)
    finally:
        log = _lib.kernel_log_end()
    assert sum(n for k, n in log.items() if k.startswith("k_hist_fill")) == 2, log
    assert np.array_equal(whole[0], plain[0])
    same_bits(q.original, plain_q.original)
    same_bits(q.final, plain_q.final)

    ubl = packing.unique_baselines(ant1, ant2)
    utime, time_inv = np.unique(tm, return_inverse=True)
    vis_w, flag_w = packing.pack_scan(time_inv.astype(np.int32), ubl, ant1, ant2, data, flags, utime.size,
                                      flagging_strategy=mode, stokes_terms=scan._stokes_terms(mode, [9, 12]))
    after = apply_strategies(strategies, flag_w, vis_w, ubl=ubl, ant_pos=None, chan_freq=freq, chan_width=width,
                             masked_channels=[])
    want_original = quality.window_histograms(vis_w, flag_w, bins, 3)
    want_final = quality.window_histograms(vis_w, after, bins, 3)
    same_counts(q.original_histograms, want_original.bl, want_original.chunk)
    same_counts(q.final_histograms, want_final.bl, want_final.chunk)
    hv, hf = (x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x) for x in (vis_w, flag_w))
    same_counts(q.original_histograms, *restate(hv, hf, bins, 3)[:2])
    # the chain moves samples from kept to flagged and leaves their slots alone
    assert np.array_equal(q.final_histograms.bl.sum(axis=2), q.original_histograms.bl.sum(axis=2))
    assert (q.final_histograms.bl[:, :, 1] >= q.original_histograms.bl[:, :, 1]).all()
    assert (q.final_histograms.chunk[:, :, 1] > q.original_histograms.chunk[:, :, 1]).any()
    assert q.final_histograms.shape == tuple(vis_w.shape) and q.final_histograms.chunk_ends.tolist() == [0, 21, 42, 64]

    qc = quality.ScanQuality(histograms=bins, freq_chunks=3)
    chunked = scan.flag_scan(data, flags, ant1, ant2, tm, freq, width, strategies, quality=qc, baseline_chunks=2, **kw)
    assert np.array_equal(chunked[0], plain[0])
    same_counts(qc.original_histograms, q.original_histograms.bl, q.original_histograms.chunk)
    same_counts(qc.final_histograms, q.final_histograms.bl, q.final_histograms.chunk)
    assert qc.final_histograms.shape == q.final_histograms.shape

    ds = dict(DATA=data, FLAG=flags, ANTENNA1=ant1, ANTENNA2=ant2, TIME=tm, CHAN_FREQ=freq, CHAN_WIDTH=width,
              FIELD_ID=0, DATA_DESC_ID=0, SCAN_NUMBER=1, CORR_TYPE=[9, 12])
    got = []
    scan.flag_scans([ds], strategies, scan_numbers=[1], flagging_strategy=mode, quality=got, histograms=bins)
    assert len(got) == 1 and got[0].final_histograms.chunk.shape[1] == 10
    assert np.array_equal(got[0].final_histograms.bl, q.final_histograms.bl)
    lines = quality.summarise_histograms(got[0].final_histograms, got[0].original_histograms)
    assert lines[3] == "Per correlation, kept samples over all chunks:" and lines[-2].strip() == "END OF HISTOGRAM SUMMARY"
