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

Beside the sums, the shape of the amplitude distribution: :func:`window_histograms`
counts the kept and the flagged samples of the windows in logarithmic amplitude
bins (:class:`AmplitudeBins`; ``tri_amplitude_histogram``, INTEGRATION.md
section 13) per window and per (corr, frequency chunk).  Integer counts merge
exactly in any order, and :class:`AmplitudeHistograms` derives quantiles, a
median-based noise level and the excess of the tail over the Rayleigh law from
them -- robust where one surviving outlier moves a ``std``.
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


class AmplitudeBins(object):
    """Logarithmic amplitude bins: ``nb = (emax - emin) << sub_bits`` bins from ``2 ** emin`` to ``2 ** emax``,
    ``2 ** sub_bits`` per octave, with ``-126 <= emin < emax <= 128``, ``0 <= sub_bits <= 5`` and at most
    ``TRI_MAX_HIST_BINS`` bins (``ValueError`` otherwise).  ``slots = nb + 3``: slot 0 is the underflow (zero
    included), slots ``1 .. nb`` are the bins, ``nb + 1`` the overflow and ``nb + 2`` the non-finite samples."""

    def __init__(self, emin=-24, emax=24, sub_bits=3):
        for name, v in (("emin", emin), ("emax", emax), ("sub_bits", sub_bits)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError("%s must be an integer, got %r" % (name, v))
        emin, emax, sub_bits = int(emin), int(emax), int(sub_bits)
        if not (-126 <= emin < emax <= 128):
            raise ValueError("bins need -126 <= emin < emax <= 128, got emin=%d, emax=%d" % (emin, emax))
        if not 0 <= sub_bits <= 5:
            raise ValueError("bins need 0 <= sub_bits <= 5, got %d" % sub_bits)
        if (emax - emin) << sub_bits > _lib.TRI_MAX_HIST_BINS:
            raise ValueError("at most %d bins, got %d" % (_lib.TRI_MAX_HIST_BINS, (emax - emin) << sub_bits))
        self.emin, self.emax, self.sub_bits = emin, emax, sub_bits
        self.nb = (emax - emin) << sub_bits
        self.slots = self.nb + 3

    def __eq__(self, other):
        return isinstance(other, AmplitudeBins) and \
            (self.emin, self.emax, self.sub_bits) == (other.emin, other.emax, other.sub_bits)

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash((self.emin, self.emax, self.sub_bits))

    def __repr__(self):
        return "AmplitudeBins(emin=%d, emax=%d, sub_bits=%d)" % (self.emin, self.emax, self.sub_bits)

    def edges(self):
        """The ``nb + 1`` bin edges, float64 and exact: bin ``k`` covers ``[edges[k], edges[k + 1])``, and
        ``edges[k] = 2 ** (emin + (k >> sub_bits)) * (1 + (k mod 2 ** sub_bits) / 2 ** sub_bits)``."""
        k = np.arange(self.nb + 1, dtype=np.int64)
        per = 1 << self.sub_bits
        return np.ldexp(1.0 + (k % per) / float(per), (self.emin + (k >> self.sub_bits)).astype(np.int32))

    def slot_of(self, amplitudes):
        """The slot of every sample, int64, by the device's rule in numpy.  float32 amplitudes (``|x|`` is taken; NaN
        and Inf are non-finite), or complex64 samples: non-finite if either part is, else the slot of the canonical
        amplitude ``float32(sqrt(float64(re) ** 2 + float64(im) ** 2))``, which may round to +Inf and then overflows."""
        x = np.asarray(amplitudes)
        if np.iscomplexobj(x):
            x = x.astype(np.complex64, copy=False)
            re_, im_ = x.real.astype(np.float64), x.imag.astype(np.float64)
            finite = np.isfinite(re_) & np.isfinite(im_)
            with np.errstate(invalid="ignore", over="ignore"):
                a = np.sqrt(re_ * re_ + im_ * im_).astype(np.float32)
        else:
            a = np.abs(x.astype(np.float32, copy=False))
            finite = np.isfinite(a)
        u = np.ascontiguousarray(a).view(np.uint32).astype(np.int64) & 0x7FFFFFFF
        k = (u >> (23 - self.sub_bits)) - ((self.emin + 127) << self.sub_bits)
        slot = np.where(k < 0, 0, np.where(k >= self.nb, self.nb + 1, k + 1))
        return np.where(finite, slot, self.nb + 2).astype(np.int64)


HIST_AXES = ("bl", "chunk")
_POPULATIONS = {0: 0, 1: 1, "kept": 0, "flagged": 1}
_RAYLEIGH_MEDIAN = float(np.sqrt(2.0 * np.log(2.0)))     # the median of a Rayleigh amplitude over its sigma


class AmplitudeHistograms(object):
    """The amplitude histograms of ``(bl, corr, time, chan)`` windows of ``shape``: ``bl`` ``(n_bl, n_corr, 2, slots)``
    int64, one cell per window, and ``chunk`` ``(n_corr, n_chunks, 2, slots)``, over baselines and times per frequency
    chunk ``[chunk_ends[g], chunk_ends[g + 1])``; population 0 are the kept samples, 1 the flagged ones, the slots are
    those of ``bins``.  The derived values are computed on the host in float64, per cell of ``axis`` ("bl" or
    "chunk"), over the slots ``0 .. nb + 1`` of one ``population`` (0 / "kept", the default, or 1 / "flagged")."""

    def __init__(self, bl, chunk, bins, chunk_ends, shape):
        self.bl, self.chunk, self.bins = bl, chunk, bins
        self.chunk_ends = np.asarray(chunk_ends, np.int64)
        self.shape = tuple(int(s) for s in shape)

    def _cells(self, axis, population):
        if axis not in HIST_AXES:
            raise ValueError("axis must be one of %s, got %r" % (", ".join(HIST_AXES), axis))
        if isinstance(population, bool) or population not in _POPULATIONS:
            raise ValueError("population must be 0 / 'kept' or 1 / 'flagged', got %r" % (population,))
        return getattr(self, axis)[:, :, _POPULATIONS[population], :self.bins.nb + 2]

    def counts(self, axis, population=0):
        """The counts of the slots ``0 .. nb + 1`` (underflow, the bins, overflow), int64 ``(cells.., nb + 2)``."""
        return self._cells(axis, population)

    def quantile(self, axis, q, population=0):
        """The ``q`` quantile of the amplitude, from the counts: with ``N`` the cell's samples and rank ``r = q * N``,
        slot ``j`` is the first non-empty one whose cumulative count reaches ``r``; the result lies in its bin
        ``[lo, hi)`` at ``lo + (hi - lo) * (r - C) / c``, ``C`` the count below the slot and ``c`` its own.  0.0 in the
        underflow, inf in the overflow, NaN where ``N`` is 0."""
        q = float(q)
        if not 0.0 <= q <= 1.0:
            raise ValueError("q must be in [0, 1], got %r" % (q,))
        c = self._cells(axis, population).astype(np.float64)
        nb = self.bins.nb
        cum = np.cumsum(c, axis=-1)
        total = cum[..., -1]
        r = q * total
        j = np.argmax((cum >= r[..., None]) & (c > 0), axis=-1)
        own = np.take_along_axis(c, j[..., None], -1)[..., 0]
        below = np.take_along_axis(cum, j[..., None], -1)[..., 0] - own
        edges = self.bins.edges()
        k = np.clip(j - 1, 0, nb - 1)
        with np.errstate(invalid="ignore", divide="ignore"):
            inside = edges[k] + (edges[k + 1] - edges[k]) * ((r - below) / own)
        out = np.where(j == 0, 0.0, np.where(j == nb + 1, np.inf, inside))
        return np.where(total > 0, out, np.nan)

    def noise_sigma(self, axis, population=0):
        """``quantile(axis, 0.5) / sqrt(2 ln 2)``: the sigma of the noise in either part if the amplitudes follow the
        Rayleigh law, whose median is ``sigma * sqrt(2 ln 2)`` -- unmoved by a tail of outliers."""
        return self.quantile(axis, 0.5, population) / _RAYLEIGH_MEDIAN

    def tail_excess(self, axis, nsigma=4.0, population=0):
        """The observed fraction of samples at or above ``e``, the first bin edge ``>= nsigma * noise_sigma``, over
        the Rayleigh law's ``exp(-(e / sigma) ** 2 / 2)``: about 1 for noise, far above 1 where RFI survives.  NaN
        where the cell is empty, its sigma is 0 or infinite, or no edge lies that high."""
        nsigma = float(nsigma)
        if not nsigma > 0.0:
            raise ValueError("nsigma must be > 0, got %r" % (nsigma,))
        c = self._cells(axis, population).astype(np.float64)
        nb = self.bins.nb
        sigma = self.noise_sigma(axis, population)
        ok = np.isfinite(sigma) & (sigma > 0)
        edges = self.bins.edges()
        first = np.searchsorted(edges, np.where(ok, nsigma * sigma, 0.0), "left")
        ok &= first <= nb
        first = np.minimum(first, nb)
        # samples at or above edges[first]: the bins first .. nb - 1 (slots first + 1 .. nb) and the overflow
        above = np.cumsum(c[..., ::-1], axis=-1)[..., ::-1]
        tail = np.take_along_axis(above, (first + 1)[..., None], -1)[..., 0]
        with np.errstate(invalid="ignore", divide="ignore", under="ignore"):
            ratio = (tail / c.sum(axis=-1)) / np.exp(-0.5 * (edges[first] / sigma) ** 2)
        return np.where(ok, ratio, np.nan)


def _hist_cap(ncorr, ntime):
    """Baselines one launch holds: at most 2^24 - 1 blocks along x, one per window and band of 64 time rows."""
    bands = -(-ntime // 64)
    return max(1, (((1 << 24) - 1) // max(bands, 1)) // max(ncorr, 1))


def window_histograms(vis_windows, flag_windows, bins=AmplitudeBins(), freq_chunks=10, *, accumulate_into=None,
                      _max_baselines=None):
    """The :class:`AmplitudeHistograms` of ``(bl, corr, time, chan)`` windows: ``vis_windows`` complex64, or float32
    amplitudes; ``flag_windows`` of the same shape, nonzero = flagged (numpy arrays or ROCm tensors).  Every sample is
    counted once, kept or flagged, in the slot of its amplitude (:class:`AmplitudeBins`); ``freq_chunks`` frequency
    chunks with the flagger's ends.

    ``accumulate_into``: the histograms of the baselines before these (same bins, chunk ends, corr, time and chan): the
    chunk cells continue from its counts, the new bl cells follow its own, and ``shape`` counts all baselines.  Counts
    are integers: the same bits on every run, for every batch size, and for a scan taken whole or in baseline ranges.
    Inputs are not modified."""
    shape = tuple(int(s) for s in vis_windows.shape)
    if len(shape) != 4:
        raise ValueError("vis_windows must be 4-D (bl, corr, time, chan), got shape %s" % (shape,))
    if tuple(int(s) for s in flag_windows.shape) != shape:
        raise ValueError("vis_windows and flag_windows must have the same shape, got %s and %s"
                         % (shape, tuple(flag_windows.shape)))
    if not isinstance(bins, AmplitudeBins):
        raise ValueError("bins must be an AmplitudeBins, got %r" % (type(bins).__name__,))
    if isinstance(freq_chunks, bool) or not isinstance(freq_chunks, (int, np.integer)) or freq_chunks < 1:
        raise ValueError("freq_chunks must be an integer >= 1, got %r" % (freq_chunks,))
    nbl, ncorr, ntime, nchan = shape
    ends, c_ends = flagging._chunk_ends(nchan, int(freq_chunks))
    nchunks = len(ends) - 1
    prev = accumulate_into
    if prev is not None:
        if not isinstance(prev, AmplitudeHistograms):
            raise ValueError("accumulate_into must be an AmplitudeHistograms, got %r" % (type(prev).__name__,))
        if prev.bins != bins:
            raise ValueError("accumulate_into holds %r, the call asks for %r" % (prev.bins, bins))
        if prev.shape[1:] != shape[1:]:
            raise ValueError("accumulate_into holds (corr, time, chan) = %s, the windows %s"
                             % (prev.shape[1:], shape[1:]))
        if not np.array_equal(prev.chunk_ends, ends):
            raise ValueError("accumulate_into holds the chunk ends %s, the call asks for %s"
                             % (prev.chunk_ends.tolist(), ends.tolist()))
    if nbl * ncorr * ntime * nchan == 0:
        # no sample: nothing for the device to do
        bl = np.zeros((nbl, ncorr, 2, bins.slots), np.int64)
        chunk = prev.chunk if prev is not None else np.zeros((ncorr, nchunks, 2, bins.slots), np.int64)
    else:
        torch = flagging._require_gpu()
        v, f8, code, _, device = flagging._as_device_inputs(torch, vis_windows, flag_windows)
        if code not in (_lib.TRI_VIS_C64, _lib.TRI_VIS_F32):
            raise TypeError("tricolour_amd.window_histograms: visibilities must be complex64 or float32")
        lib = _lib.lib()
        if prev is None:
            h_chunk = torch.empty((ncorr, nchunks, 2, bins.slots), dtype=torch.int64, device=device)
        else:
            h_chunk = torch.from_numpy(np.ascontiguousarray(prev.chunk, dtype=np.int64)).to(device)
        parts = []
        with torch.cuda.device(device):
            launches, tail = flagging._window_launches(torch, device, nbl, lambda b: 0, _hist_cap(ncorr, ntime),
                                                       _max_baselines, workspace=False)
            accumulate = prev is not None
            for at, b in launches:
                h_bl = torch.empty((b, ncorr, 2, bins.slots), dtype=torch.int64, device=device)
                _lib.check(lib.tri_amplitude_histogram(at(v), code, at(f8), b, ncorr, ntime, nchan, c_ends, len(ends),
                                                       bins.emin, bins.emax, bins.sub_bits, h_bl.data_ptr(),
                                                       h_chunk.data_ptr(), 1 if accumulate else 0, tail[2]))
                parts.append(h_bl)
                accumulate = True
        bl = np.concatenate([p.cpu().numpy() for p in parts])
        chunk = h_chunk.cpu().numpy()
    if prev is not None:
        bl = np.concatenate([prev.bl, bl])
        nbl += prev.shape[0]
    return AmplitudeHistograms(bl, chunk, bins, ends, (nbl, ncorr, ntime, nchan))


def summarise_histograms(final, original):
    """The histogram summary as text lines, in the manner of :func:`summarise_quality`: per corr, over all chunks,
    the noise sigma and the tail excess of the kept samples after and before flagging; the chunks whose tail excess
    after flagging stands out (above ``median + 5 * 1.4826 * MAD`` over the corr's chunks); and the median amplitude of
    what the chain flagged (the flagged samples after minus those before)."""
    bar = "**********************************"
    lines = [bar, "  BEGINNING OF HISTOGRAM SUMMARY  ", bar, "Per correlation, kept samples over all chunks:"]
    ncorr = final.shape[1]

    def whole(h, chunk):
        # one cell per corr: the chunk cells summed
        return AmplitudeHistograms(h.bl[:0], chunk.sum(axis=1, keepdims=True), h.bins, h.chunk_ends[[0, -1]], h.shape)

    after, before = whole(final, final.chunk), whole(original, original.chunk)
    for corr in range(ncorr):
        cells = ["noise sigma {0:.4g}, original {1:.4g}".format(float(after.noise_sigma("chunk")[corr, 0]),
                                                                float(before.noise_sigma("chunk")[corr, 0])),
                 "tail excess {0:.4g}, original {1:.4g}".format(float(after.tail_excess("chunk")[corr, 0]),
                                                                float(before.tail_excess("chunk")[corr, 0]))]
        lines.append("\t {0:d}: {1:s}".format(corr, "; ".join(cells)))
    lines.append("Chunks whose tail excess stands out:")
    excess = final.tail_excess("chunk")
    for corr in range(ncorr):
        line = excess[corr]
        ok = ~np.isnan(line)
        mine = np.zeros(0, np.int64)
        if ok.any():
            med = np.median(line[ok])
            mad = np.median(np.abs(line[ok] - med))
            with np.errstate(invalid="ignore"):
                mine = np.flatnonzero(ok & (line > med + 5.0 * 1.4826 * mad))
        lines.append("\t {0:d}: {1:s}".format(corr, " ".join(str(int(i)) for i in mine) if mine.size else "none"))
    lines.append("Median amplitude of what the chain flagged:")
    # the chain only adds flags over the same samples: a sample moves from kept to flagged, its slot stays
    gone = np.maximum(final.chunk[:, :, 1] - original.chunk[:, :, 1], 0)
    taken = np.stack([np.zeros_like(gone), gone], axis=2)
    removed = whole(final, taken)
    for corr in range(ncorr):
        n = int(removed.counts("chunk", 1)[corr, 0].sum())
        lines.append("\t {0:d}: {1:.4g} ({2:d} samples)".format(corr, float(removed.quantile("chunk", 0.5, 1)[corr, 0]), n))
    lines += [bar, "     END OF HISTOGRAM SUMMARY     ", bar]
    return lines


class ScanQuality(object):
    """What ``flag_scan(..., quality=ScanQuality())`` fills in place: the :class:`QualityStatistics` of the scan's
    packed windows under the flags before (``original``) and after (``final``) the strategy chain, the ``ubl`` rows
    the ``bl`` cells belong to, ``chan_freq`` and the scan's unique ``times``.

    ``histograms``: None, or the :class:`AmplitudeBins` with which the :class:`AmplitudeHistograms` of the same windows
    are taken as well, with ``freq_chunks`` frequency chunks: ``original_histograms`` and ``final_histograms``."""

    def __init__(self, histograms=None, freq_chunks=10):
        if histograms is not None and not isinstance(histograms, AmplitudeBins):
            raise ValueError("histograms must be None or an AmplitudeBins, got %r" % (type(histograms).__name__,))
        if isinstance(freq_chunks, bool) or not isinstance(freq_chunks, (int, np.integer)) or freq_chunks < 1:
            raise ValueError("freq_chunks must be an integer >= 1, got %r" % (freq_chunks,))
        self.original = None
        self.final = None
        self.ubl = None
        self.chan_freq = None
        self.times = None
        self.histograms = histograms
        self.freq_chunks = int(freq_chunks)
        self.original_histograms = None
        self.final_histograms = None
