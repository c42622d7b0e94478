"""Quality statistics of the visibilities that survive flagging: count, sum and
sum of squares of the unflagged samples per baseline, per timestep and per
channel, plus a differential noise estimate from neighbouring channels that the
sky does not enter (after AOFlagger's quality statistics; the definition is
this library's own, INTEGRATION.md section 12 and ``include/tricolour_amd.h``).

A measurement beside the strategy chain, like
:mod:`tricolour_amd.window_statistics`, not a strategy task:
:func:`window_quality` takes the statistics of ``(bl, corr, time, chan)``
windows on the device (``tri_window_quality``, one pass over the slab),
:class:`QualityStatistics` derives mean, scatter, differential scatter, their
ratio and the occupancy from them on the host, and ``flag_scan(...,
quality=ScanQuality())`` fills both for the windows before and after a chain.
Importing this module needs neither torch nor a GPU.
"""
import collections

import numpy as np

from tricolour_amd import _lib, flagging

AxisQuality = collections.namedtuple("AxisQuality", "n sum_re sum_im sum_p dn dsum_p")
AxisQuality.__doc__ = """The six numbers of every cell of one grouping, numpy arrays of one shape: ``n`` valid
samples and ``dn`` valid channel pairs (int64), the sums of the valid samples' parts ``sum_re`` / ``sum_im``, of their
power ``sum_p`` and of the pairs' squared differences ``dsum_p`` (float64)."""

AXES = ("bl", "time", "chan")
_DERIVED = ("mean", "std", "dstd", "excess", "occupancy")


def _ratio(a, b):
    """``a / b`` elementwise, NaN where ``b`` is 0."""
    a = np.asarray(a)
    out = np.full(a.shape, np.nan, dtype=np.result_type(a.dtype, np.float64))
    np.divide(a, b, out=out, where=np.asarray(b) != 0)
    return out


class QualityStatistics(object):
    """The statistics of ``(bl, corr, time, chan)`` windows of ``shape``: the :class:`AxisQuality` of the groupings
    ``bl`` (cells ``(bl, corr)``, over time and chan), ``time`` (``(corr, time)``, over bl and chan) and ``chan``
    (``(corr, chan)``, over bl and time)."""

    def __init__(self, bl, time, chan, shape):
        self.bl, self.time, self.chan = bl, time, chan
        self.shape = tuple(int(s) for s in shape)

    def _axis(self, axis):
        if axis not in AXES:
            raise ValueError("axis must be one of %s, got %r" % (", ".join(AXES), axis))
        return getattr(self, axis)

    def size(self, axis):
        """Samples per cell of the grouping."""
        self._axis(axis)
        nbl, ncorr, ntime, nchan = self.shape
        return {"bl": ntime * nchan, "time": nbl * nchan, "chan": nbl * ntime}[axis]

    def mean(self, axis):
        """``(sum_re + 1j * sum_im) / n``; NaN where ``n`` is 0."""
        a = self._axis(axis)
        return _ratio(a.sum_re + 1j * a.sum_im, a.n)

    def std(self, axis):
        """``sqrt(max(sum_p / n - |mean|^2, 0))``; NaN where ``n`` is 0."""
        a = self._axis(axis)
        m = self.mean(axis)
        return np.sqrt(np.maximum(_ratio(a.sum_p, a.n) - (m.real * m.real + m.imag * m.imag), 0.0))

    def dstd(self, axis):
        """``sqrt(dsum_p / (2 * dn))``: the per-sample scatter if neighbouring channels hold the same signal; NaN
        where ``dn`` is 0."""
        a = self._axis(axis)
        return np.sqrt(_ratio(a.dsum_p, 2 * a.dn))

    def excess(self, axis):
        """``std / dstd``: about 1 for noise, far above 1 where signal or RFI survives."""
        return _ratio(self.std(axis), self.dstd(axis))

    def occupancy(self, axis):
        """``1 - n / size``: the fraction of the cell's samples that are not valid; NaN where ``n`` is 0, like every
        derived value (a cell nothing is left of has no statistics, and it is never an outlier)."""
        a = self._axis(axis)
        size = self.size(axis)
        out = np.full(a.n.shape, np.nan)
        np.subtract(1.0, a.n / float(max(size, 1)), out=out, where=a.n != 0)
        return out

    def outliers(self, axis, what="dstd", nsigma=5.0):
        """Indices (a ``(k, 2)`` int array, rows in the grouping's cell order) of the cells whose ``what`` lies above
        ``median + nsigma * 1.4826 * MAD`` of ``what`` over the grouping, per corr.  NaN cells are left out of the
        median and never reported."""
        if what not in _DERIVED or what == "mean":
            raise ValueError("what must be one of std, dstd, excess, occupancy, got %r" % (what,))
        nsigma = float(nsigma)
        if not nsigma >= 0.0:
            raise ValueError("nsigma must be >= 0, got %r" % (nsigma,))
        v = getattr(self, what)(axis)
        corr_axis = 1 if axis == "bl" else 0
        hit = np.zeros(v.shape, bool)
        for corr in range(v.shape[corr_axis]):
            line = np.take(v, corr, axis=corr_axis)
            ok = ~np.isnan(line)
            if not ok.any():
                continue
            med = np.median(line[ok])
            mad = np.median(np.abs(line[ok] - med))
            with np.errstate(invalid="ignore"):
                over = ok & (line > med + nsigma * 1.4826 * mad)
            if axis == "bl":
                hit[:, corr] = over
            else:
                hit[corr] = over
        return np.argwhere(hit)


def _empty_axis(shape):
    return AxisQuality(np.zeros(shape, np.int64), np.zeros(shape), np.zeros(shape), np.zeros(shape),
                       np.zeros(shape, np.int64), np.zeros(shape))


def _axis_from(counts, sums, shape):
    return AxisQuality(counts[0].reshape(shape), sums[0].reshape(shape), sums[1].reshape(shape), sums[2].reshape(shape),
                       counts[1].reshape(shape), sums[3].reshape(shape))


def _quality_cap(ncorr, ntime, nchan):
    """Baselines one launch holds: fewer than 2^31 blocks, one per window and group of 4 strips of 256 channels."""
    groups = -(-(-(-nchan // 256)) // 4)
    return max(1, (((1 << 31) - 1) // max(groups, 1)) // max(ncorr, 1))


def window_quality(vis_windows, flag_windows, *, accumulate_into=None, _max_baselines=None):
    """The :class:`QualityStatistics` of ``(bl, corr, time, chan)`` windows: ``vis_windows`` complex64, or float32
    amplitudes; ``flag_windows`` of the same shape, nonzero = flagged (numpy arrays or ROCm tensors).  A sample is
    valid if it is unflagged and both parts are finite.

    ``accumulate_into``: the statistics of the baselines before these (same corr, time and chan): the time and chan
    cells continue from its values, the new bl cells follow its own, and ``shape`` counts all baselines.  The sums run
    in a fixed order, the time and chan cells adding baselines one after the other: the same bits on every run, for
    every batch size, and for a scan taken whole or in consecutive baseline ranges.  Inputs are not modified."""
    shape = tuple(int(s) for s in vis_windows.shape)
    if len(shape) != 4:
        raise ValueError("vis_windows must be 4-D (bl, corr, time, chan), got shape %s" % (shape,))
    if tuple(int(s) for s in flag_windows.shape) != shape:
        raise ValueError("vis_windows and flag_windows must have the same shape, got %s and %s"
                         % (shape, tuple(flag_windows.shape)))
    nbl, ncorr, ntime, nchan = shape
    if accumulate_into is not None:
        if not isinstance(accumulate_into, QualityStatistics):
            raise ValueError("accumulate_into must be a QualityStatistics, got %r" % (type(accumulate_into).__name__,))
        if accumulate_into.shape[1:] != shape[1:]:
            raise ValueError("accumulate_into holds (corr, time, chan) = %s, the windows %s"
                             % (accumulate_into.shape[1:], shape[1:]))
    prev = accumulate_into
    if nbl * ncorr * ntime * nchan == 0:
        # no sample: nothing for the device to do
        bl = _empty_axis((nbl, ncorr))
        time = prev.time if prev is not None else _empty_axis((ncorr, ntime))
        chan = prev.chan if prev is not None else _empty_axis((ncorr, nchan))
    else:
        torch = flagging._require_gpu()
        v, f8, code, _, device = flagging._as_device_inputs(torch, vis_windows, flag_windows)
        if code not in (_lib.TRI_VIS_C64, _lib.TRI_VIS_F32):
            raise TypeError("tricolour_amd.window_quality: visibilities must be complex64 or float32")
        lib = _lib.lib()

        def dev(host, dtype, rows, cells):
            if host is None:
                return torch.empty((rows, cells), dtype=dtype, device=device)
            return torch.from_numpy(np.ascontiguousarray(np.stack([a.reshape(-1) for a in host]))).to(device)

        pt, pc = (None, None) if prev is None else (prev.time, prev.chan)
        cnt_t = dev(pt and (pt.n, pt.dn), torch.int64, 2, ncorr * ntime)
        sum_t = dev(pt and (pt.sum_re, pt.sum_im, pt.sum_p, pt.dsum_p), torch.float64, 4, ncorr * ntime)
        cnt_c = dev(pc and (pc.n, pc.dn), torch.int64, 2, ncorr * nchan)
        sum_c = dev(pc and (pc.sum_re, pc.sum_im, pc.sum_p, pc.dsum_p), torch.float64, 4, ncorr * nchan)
        parts = []
        with torch.cuda.device(device):
            launches, tail = flagging._window_launches(
                torch, device, nbl, lambda b: lib.tri_quality_workspace_bytes(b, ncorr, ntime, nchan),
                _quality_cap(ncorr, ntime, nchan), _max_baselines)
            accumulate = prev is not None
            for at, b in launches:
                cnt_b = torch.empty((2, b * ncorr), dtype=torch.int64, device=device)
                sum_b = torch.empty((4, b * ncorr), dtype=torch.float64, device=device)
                _lib.check(lib.tri_window_quality(at(v), code, at(f8), b, ncorr, ntime, nchan, cnt_b.data_ptr(),
                                                  sum_b.data_ptr(), cnt_t.data_ptr(), sum_t.data_ptr(), cnt_c.data_ptr(),
                                                  sum_c.data_ptr(), 1 if accumulate else 0, *tail))
                parts.append((cnt_b, sum_b, b))
                accumulate = True
        bl = AxisQuality(*(np.concatenate(cols) for cols in zip(*(
            _axis_from(c.cpu().numpy(), s.cpu().numpy(), (b, ncorr)) for c, s, b in parts))))
        time = _axis_from(cnt_t.cpu().numpy(), sum_t.cpu().numpy(), (ncorr, ntime))
        chan = _axis_from(cnt_c.cpu().numpy(), sum_c.cpu().numpy(), (ncorr, nchan))
    if prev is not None:
        bl = AxisQuality(*(np.concatenate([a, b]) for a, b in zip(prev.bl, bl)))
        nbl += prev.shape[0]
    return QualityStatistics(bl, time, chan, (nbl, ncorr, ntime, nchan))


def _nanmedian(v):
    v = v[~np.isnan(v)]
    return float(np.median(v)) if v.size else float("nan")


def summarise_quality(final, original):
    """The quality summary as text lines, in the manner of ``summarise_stats``: per corr the median differential
    scatter, the median excess and the occupancy over channels after and before flagging, then the outlying baselines,
    timesteps and channels (in ``dstd``) after flagging."""
    bar = "********************************"
    lines = [bar, "  BEGINNING OF QUALITY SUMMARY  ", bar, "Per correlation, over channels:"]
    ncorr = final.shape[1]
    for corr in range(ncorr):
        cells = []
        for what in ("dstd", "excess"):
            cells.append("median {0:s} {1:.4g}, original {2:.4g}".format(
                what, _nanmedian(getattr(final, what)("chan")[corr]), _nanmedian(getattr(original, what)("chan")[corr])))
        occ = []
        for stats in (final, original):
            n, size = int(stats.chan.n[corr].sum()), stats.size("chan") * stats.shape[3]
            occ.append(100.0 * (1.0 - n / size) if size else float("nan"))
        cells.append("occupancy {0:.3f}%, original {1:.3f}%".format(*occ))
        lines.append("\t {0:d}: {1:s}".format(corr, "; ".join(cells)))
    for title, axis in (("Outlying baselines (row of ubl):", "bl"), ("Outlying timesteps:", "time"),
                        ("Outlying channels:", "chan")):
        lines.append(title)
        found = final.outliers(axis)
        column = 0 if axis == "bl" else 1
        for corr in range(ncorr):
            mine = found[found[:, 1 - column] == corr][:, column]
            lines.append("\t {0:d}: {1:s}".format(corr, " ".join(str(int(i)) for i in mine) if mine.size else "none"))
    lines += [bar, "     END OF QUALITY SUMMARY     ", bar]
    return lines


class ScanQuality(object):
    """What ``flag_scan(..., quality=ScanQuality())`` fills in place: the :class:`QualityStatistics` of the scan's
    packed windows under the flags before (``original``) and after (``final``) the strategy chain, the ``ubl`` rows
    the ``bl`` cells belong to, ``chan_freq`` and the scan's unique ``times``."""

    def __init__(self):
        self.original = None
        self.final = None
        self.ubl = None
        self.chan_freq = None
        self.times = None
