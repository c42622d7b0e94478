"""Quality statistics of the unflagged samples (tricolour_amd.quality, tri_window_quality)
against a host restatement whose sums carry no summation error.

restate_quality() is numpy float64 per the definition, every cell summed with math.fsum.  Dyadic inputs (parts are
integers in [-512, 512] divided by 8) make every term and every partial sum of every cell exactly representable, so the
device must give the restatement's bits whatever its order; Gaussian inputs are held to a derived bound; the order
contract (batches, accumulate, runs) is tested bit for bit on Gaussian inputs, where the order shows."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

from tricolour_amd import quality
from tricolour_amd.quality import AxisQuality, QualityStatistics

HPP = os.path.join(ROOT, "tricolour_amd", "csrc", "steps", "quality", "kernels_quality.hpp")
FIELDS = AxisQuality._fields
SUMS = ("sum_re", "sum_im", "sum_p", "dsum_p")


def header_constants():
    """The QUAL_* constants of the kernel header, evaluated."""
    out = {}
    with open(HPP) as fh:
        for name, expr in re.findall(r"^#define[ \t]+(QUAL_\w+)[ \t]+(.+?)[ \t]*(?://.*)?$", fh.read(), re.M):
            out[name] = int(eval(expr, {"__builtins__": {}}, dict(out)))
    return out


Q = header_constants()
V, SW, WPB, ROWS, NT = Q["QUAL_V"], Q["QUAL_SW"], Q["QUAL_WPB"], Q["QUAL_ROWS"], Q["QUAL_NT"]


# ---- the restatement ----

def sample_terms(vis, flags):
    """Per sample, float64: validity, the parts, p; per pair (stored at its channel c): validity and dp."""
    vis = np.asarray(vis)
    re_ = vis.real.astype(np.float64)
    im_ = vis.imag.astype(np.float64) if np.iscomplexobj(vis) else np.zeros(vis.shape)
    ok = (np.asarray(flags) == 0) & np.isfinite(re_) & np.isfinite(im_)
    p = re_ * re_ + im_ * im_
    pair = np.zeros(vis.shape, bool)
    dp = np.zeros(vis.shape)
    if vis.shape[-1] > 1:
        pair[..., :-1] = ok[..., :-1] & ok[..., 1:]
        with np.errstate(invalid="ignore"):
            dre = re_[..., 1:] - re_[..., :-1]
            dim = im_[..., 1:] - im_[..., :-1]
            dp[..., :-1] = dre * dre + dim * dim
    return ok, re_, im_, p, pair, dp


def _cells(a, keep):
    """``a`` (bl, corr, time, chan) as (cells, terms): the axes ``keep`` first, in that order."""
    rest = tuple(i for i in range(4) if i not in keep)
    shape = tuple(a.shape[i] for i in keep)
    return np.transpose(a, keep + rest).reshape(int(np.prod(shape, dtype=np.int64)), -1), shape


def _fsum_cells(values, valid, keep, absolute=False):
    v = np.where(valid, np.abs(values) if absolute else values, 0.0)
    rows, shape = _cells(v, keep)
    return np.array([math.fsum(r) for r in rows.tolist()], np.float64).reshape(shape)


KEEP = {"bl": (0, 1), "time": (1, 2), "chan": (1, 3)}


def restate_quality(vis, flags, absolute=False):
    """The QualityStatistics of the definition; ``absolute``: the sums of the terms' absolute values instead."""
    ok, re_, im_, p, pair, dp = sample_terms(vis, flags)
    axes = {}
    for axis, keep in KEEP.items():
        n = _cells(ok, keep)[0].sum(axis=1, dtype=np.int64).reshape(_cells(ok, keep)[1])
        dn = _cells(pair, keep)[0].sum(axis=1, dtype=np.int64).reshape(n.shape)
        axes[axis] = AxisQuality(n, _fsum_cells(re_, ok, keep, absolute), _fsum_cells(im_, ok, keep, absolute),
                                 _fsum_cells(p, ok, keep, absolute), dn, _fsum_cells(dp, pair, keep, absolute))
    return QualityStatistics(axes["bl"], axes["time"], axes["chan"], np.asarray(vis).shape)


def same_bits(a, b):
    assert a.shape == b.shape
    for axis in quality.AXES:
        for name in FIELDS:
            x, y = getattr(getattr(a, axis), name), getattr(getattr(b, axis), name)
            assert x.dtype == y.dtype and x.shape == y.shape, (axis, name, x.dtype, y.dtype, x.shape, y.shape)
            assert np.array_equal(x, y), (axis, name, int((x != y).sum()))


def dyadic(shape, seed, dtype="c64"):
    rs = np.random.RandomState(seed)
    re_ = (rs.randint(-512, 513, shape) / 8.0).astype(np.float32)
    if dtype == "f32":
        return re_
    return (re_ + 1j * (rs.randint(-512, 513, shape) / 8.0)).astype(np.complex64)


def gaussian(shape, seed):
    rs = np.random.RandomState(seed)
    return (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(np.complex64)


def random_flags(shape, seed, frac=0.2):
    return np.random.RandomState(seed).random_sample(shape) < frac


# ---- CPU: the restatement on hand-made windows ----

def test_restatement_one_flagged_sample():
    vis = np.array([[1 + 2j, 3 + 4j, 5 + 6j], [7 + 8j, 9 + 10j, 11 + 12j]], np.complex64)[None, None]
    flags = np.zeros(vis.shape, bool)
    flags[0, 0, 0, 1] = True
    s = restate_quality(vis, flags)
    assert s.bl.n.tolist() == [[5]] and s.bl.dn.tolist() == [[2]]
    assert s.bl.sum_re.tolist() == [[1 + 5 + 7 + 9 + 11.0]] and s.bl.sum_im.tolist() == [[2 + 6 + 8 + 10 + 12.0]]
    assert s.bl.sum_p.tolist() == [[5 + 61 + 113 + 181 + 265.0]] and s.bl.dsum_p.tolist() == [[16.0]]
    assert s.time.n.tolist() == [[2, 3]] and s.time.dn.tolist() == [[0, 2]] and s.time.dsum_p.tolist() == [[0.0, 16.0]]
    assert s.chan.n.tolist() == [[2, 1, 2]] and s.chan.dn.tolist() == [[1, 1, 0]]
    assert s.chan.sum_re.tolist() == [[8.0, 9.0, 16.0]] and s.chan.dsum_p.tolist() == [[8.0, 8.0, 0.0]]


def test_restatement_nonfinite_samples_do_not_count_and_break_their_pairs():
    vis = np.ones((1, 1, 2, 5), np.complex64)
    vis[0, 0, 0, 1] = np.nan
    vis[0, 0, 1, 3] = np.inf + 1j
    s = restate_quality(vis, np.zeros(vis.shape, np.uint8))
    assert s.bl.n.tolist() == [[8]] and s.bl.dn.tolist() == [[4]]
    assert s.chan.n.tolist() == [[2, 1, 2, 1, 2]] and s.chan.dn.tolist() == [[1, 1, 1, 1, 0]]
    assert s.time.n.tolist() == [[4, 4]] and s.time.dn.tolist() == [[2, 2]]
    for axis in quality.AXES:
        for name in SUMS:
            assert np.isfinite(getattr(getattr(s, axis), name)).all()
    assert s.bl.sum_re.tolist() == [[8.0]] and s.bl.sum_p.tolist() == [[8.0]] and s.bl.dsum_p.tolist() == [[0.0]]


def test_restatement_single_channel_has_no_pairs():
    s = restate_quality(dyadic((2, 2, 3, 1), 1), np.zeros((2, 2, 3, 1), bool))
    for axis in quality.AXES:
        assert not getattr(s, axis).dn.any() and not getattr(s, axis).dsum_p.any()
    assert s.chan.n.tolist() == [[6], [6]]


def test_dyadic_inputs_do_not_depend_on_the_summation_order():
    """Every partial sum of every cell is exact: two orders, one result."""
    vis, flags = dyadic((3, 2, 9, 130), 2), random_flags((3, 2, 9, 130), 3)
    ok, re_, im_, p, pair, dp = sample_terms(vis, flags)
    s = restate_quality(vis, flags)
    for values, valid, name in ((re_, ok, "sum_re"), (im_, ok, "sum_im"), (p, ok, "sum_p"), (dp, pair, "dsum_p")):
        v = np.where(valid, values, 0.0)
        forward = np.add.reduce(np.add.reduce(v, axis=3), axis=2)
        backward = np.add.reduce(np.add.reduce(v[:, :, ::-1, ::-1], axis=2), axis=2)
        assert np.array_equal(forward, getattr(s.bl, name)) and np.array_equal(backward, getattr(s.bl, name))


# ---- CPU: derived values, outliers, summary ----

def test_derived_values_are_nan_where_empty():
    vis, flags = dyadic((2, 1, 3, 4), 4), np.zeros((2, 1, 3, 4), bool)
    flags[1] = True                     # baseline 1 is empty
    flags[0, 0, :, 2] = True            # so is channel 2; channel 1 keeps its samples and loses its pairs
    s = restate_quality(vis, flags)
    for what in ("mean", "std", "dstd", "excess", "occupancy"):
        assert np.isnan(getattr(s, what)("bl")[1, 0]) and not np.isnan(getattr(s, what)("bl")[0, 0]), what
        assert np.isnan(getattr(s, what)("chan")[0, 2]), what
    assert s.chan.n[0, 1] == 3 and s.chan.dn[0, 1] == 0
    assert np.isnan(s.dstd("chan")[0, 1]) and np.isnan(s.excess("chan")[0, 1]) and not np.isnan(s.std("chan")[0, 1])
    n, a = s.bl.n[0, 0], s.bl
    mean = (a.sum_re[0, 0] + 1j * a.sum_im[0, 0]) / n
    assert s.mean("bl")[0, 0] == mean
    assert s.std("bl")[0, 0] == np.sqrt(max(a.sum_p[0, 0] / n - abs(mean) ** 2, 0.0))
    assert s.dstd("bl")[0, 0] == np.sqrt(a.dsum_p[0, 0] / (2 * a.dn[0, 0]))
    assert s.occupancy("bl")[0, 0] == 1 - 9 / 12.0 and s.occupancy("time")[0, 0] == 1 - 3 / 8.0
    assert s.excess("bl")[0, 0] == s.std("bl")[0, 0] / s.dstd("bl")[0, 0]
    assert s.outliers("bl").shape == (0, 2)                                            # NaN cells are never reported
    with pytest.raises(ValueError):
        s.outliers("corr")
    with pytest.raises(ValueError):
        s.outliers("bl", what="mean")


@pytest.mark.parametrize("axis, index", [("bl", 4), ("time", 7), ("chan", 21)])
def test_outliers_report_the_planted_cell_and_nothing_else(axis, index):
    vis = gaussian((9, 2, 12, 40), 5)
    where = {"bl": np.s_[index], "time": np.s_[:, :, index], "chan": np.s_[..., index]}[axis]
    vis[where] *= np.float32(6)
    s = restate_quality(vis, random_flags(vis.shape, 6, 0.1))
    got = s.outliers(axis, "std")
    want = [[index, 0], [index, 1]] if axis == "bl" else [[0, index], [1, index]]
    assert got.tolist() == want
    if axis != "chan":                  # (a loud channel also raises the differences of the pair of the channel before it)
        assert s.outliers(axis, "dstd").tolist() == want
    if axis == "bl":                    # noise, quiet or loud: std / dstd is about 1
        assert np.all(np.abs(s.excess("bl") - 1.0) < 0.25)


def _hand_stats(scale):
    """2 baselines, 1 corr, 2 times, 3 channels, every sample valid and (scale, 0) except channel 1 = (3 * scale, 0)."""
    vis = np.full((2, 1, 2, 3), scale, np.complex64)
    vis[..., 1] *= 3
    flags = np.zeros(vis.shape, bool)
    if scale == 1:
        flags[0, 0, 0, 0] = True
    return restate_quality(vis, flags)


def test_summarise_quality_text():
    lines = quality.summarise_quality(_hand_stats(1), _hand_stats(2))
    bar = "********************************"
    assert lines == [
        bar, "  BEGINNING OF QUALITY SUMMARY  ", bar,
        "Per correlation, over channels:",
        "\t 0: median dstd 1.414, original 2.828; median excess 0, original 0; occupancy 8.333%, original 0.000%",
        "Outlying baselines (row of ubl):", "\t 0: none",
        "Outlying timesteps:", "\t 0: none",
        "Outlying channels:", "\t 0: none",
        bar, "     END OF QUALITY SUMMARY     ", bar]


def test_summarise_quality_lists_outliers():
    vis = gaussian((9, 2, 12, 40), 7)
    vis[4] *= np.float32(6)
    flags = np.zeros(vis.shape, bool)
    lines = quality.summarise_quality(restate_quality(vis, flags), restate_quality(vis, flags))
    at = lines.index("Outlying baselines (row of ubl):")
    assert lines[at + 1:at + 3] == ["\t 0: 4", "\t 1: 4"]
    assert lines[lines.index("Outlying timesteps:") + 1] == "\t 0: none"


# ---- CPU: argument errors, ABI, import ----

def test_window_quality_argument_errors_come_before_any_device_work():
    vis = np.zeros((2, 1, 3, 4), np.complex64)
    with pytest.raises(ValueError, match="4-D"):
        quality.window_quality(vis[0], np.zeros((1, 3, 4), bool))
    with pytest.raises(ValueError, match="same shape"):
        quality.window_quality(vis, np.zeros((2, 1, 3, 5), bool))
    with pytest.raises(ValueError, match="QualityStatistics"):
        quality.window_quality(vis, np.zeros(vis.shape, bool), accumulate_into=object())
    other = restate_quality(np.zeros((1, 1, 3, 5), np.complex64), np.zeros((1, 1, 3, 5), bool))
    with pytest.raises(ValueError, match="corr, time, chan"):
        quality.window_quality(vis, np.zeros(vis.shape, bool), accumulate_into=other)


def test_empty_windows_need_no_device():
    s = quality.window_quality(np.zeros((0, 2, 3, 4), np.complex64), np.zeros((0, 2, 3, 4), bool))
    assert s.shape == (0, 2, 3, 4) and s.bl.n.shape == (0, 2) and s.time.n.shape == (2, 3) and s.chan.sum_p.shape == (2, 4)
    assert s.time.n.dtype == np.int64 and s.chan.dsum_p.dtype == np.float64 and not s.chan.n.any()
    prev = restate_quality(dyadic((2, 2, 3, 4), 8), np.zeros((2, 2, 3, 4), bool))
    same_bits(quality.window_quality(np.zeros((0, 2, 3, 4), np.complex64), np.zeros((0, 2, 3, 4), bool),
                                     accumulate_into=prev), prev)


def test_flag_scan_rejects_a_wrong_quality_object_before_any_device_work():
    from tricolour_amd import scan
    data = np.zeros((4, 8, 2), np.complex64)
    args = (data, np.zeros(data.shape, bool), np.zeros(4, np.int32), np.ones(4, np.int32), np.arange(4.0),
            np.linspace(1e9, 1.1e9, 8), np.full(8, 1e6), [{"task": "flag_autos"}])
    for wrong in (object(), [], "yes", quality.QualityStatistics):
        with pytest.raises(ValueError, match="ScanQuality"):
            scan.flag_scan(*args, quality=wrong)
    with pytest.raises(ValueError, match="list"):
        scan.flag_scans([], [{"task": "flag_autos"}], quality=quality.ScanQuality())


def test_abi_declares_and_exports_the_entry_points():
    from tricolour_amd import _lib
    hdr = open(_lib.HEADER).read()
    for name in ("tri_quality_workspace_bytes", "tri_window_quality"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().tri_version() >= 107
    assert HPP in _lib.DEPENDS


def test_abi_workspace_bytes():
    from tricolour_amd import _lib
    ws = _lib.lib().tri_quality_workspace_bytes
    one = ws(1, 1, 1024, 4096)
    assert 0 < one < 0.03 * 1024 * 4096 * 8                                            # low percent of the window
    assert one < ws(2, 1, 1024, 4096) <= 2 * one and ws(1, 2, 1024, 4096) == ws(2, 1, 1024, 4096)
    for shape in ((0, 1, 4, 4), (1, 0, 4, 4), (1, 1, 0, 4), (1, 1, 4, 0), (-1, 1, 4, 4), (1, 1, 1 << 31, 4),
                  (1, 1, 4, 1 << 31), (1 << 31, 1, 4, 4), (1 << 20, 1 << 20, 4, 4)):
        assert ws(*shape) == 0, shape


def test_abi_rejects_bad_arguments_without_a_launch():
    from tricolour_amd import _lib
    lib = _lib.lib()
    buf = (C.c_uint8 * (16 * 4096))()
    base = C.addressof(buf)
    v, f, ws, cb, sb, ct, st, cc, sc = (base + 4096 * i for i in range(9))

    def call(vis=v, dtype=_lib.TRI_VIS_C64, flags=f, n_bl=2, n_corr=2, ntime=4, nchan=8, cb=cb, sb=sb, ct=ct, st=st, cc=cc,
             sc=sc, acc=0, ws=ws, wsb=0):
        return lib.tri_window_quality(vis, dtype, flags, n_bl, n_corr, ntime, nchan, cb, sb, ct, st, cc, sc, acc, ws, wsb,
                                      None)
    for name in ("vis", "flags", "cb", "sb", "ct", "st", "cc", "sc"):
        assert call(**{name: None}) == _lib.TRI_EINVAL, name
    for name in ("n_bl", "n_corr", "ntime", "nchan"):
        assert call(**{name: -1}) == _lib.TRI_EINVAL, name
    for dt in (_lib.TRI_VIS_C128, _lib.TRI_VIS_F64, 17, -1):
        assert call(dtype=dt) == _lib.TRI_EINVAL, dt
    # outputs over an input, over each other
    for kw in (dict(cb=v + 8), dict(sb=f), dict(ct=v + 1000), dict(st=cb), dict(cc=sb + 8), dict(sc=cc), dict(sc=st + 16),
               dict(cc=f + 100)):
        assert call(**kw) == _lib.TRI_EINVAL, kw
    assert b"overlap" in lib.tri_last_error()
    assert call() == _lib.TRI_EWORKSPACE and call(ws=None, wsb=1 << 30) == _lib.TRI_EWORKSPACE
    need = lib.tri_quality_workspace_bytes(2, 2, 4, 8)
    assert call(wsb=need - 1) == _lib.TRI_EWORKSPACE
    for kw in (dict(ntime=1 << 31), dict(nchan=1 << 31), dict(n_bl=1 << 31), dict(n_bl=1 << 20, n_corr=1 << 20)):
        assert call(**kw) == _lib.TRI_EUNSUPPORTED, kw
    # an empty shape that leaves nothing to write: no launch, no device
    assert call(n_corr=0) == _lib.TRI_OK
    assert call(n_bl=0, acc=1) == _lib.TRI_OK
    # argument errors win over the empty shape
    assert call(n_bl=0, vis=None) == _lib.TRI_EINVAL and call(n_corr=0, dtype=9) == _lib.TRI_EINVAL


def test_importing_the_module_needs_no_torch():
    code = "import sys; import tricolour_amd.quality; assert 'torch' not in sys.modules, 'torch was imported'"
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True, timeout=120)


def test_scan_quality_is_a_plain_holder():
    q = quality.ScanQuality()
    assert (q.original, q.final, q.ubl, q.chan_freq, q.times) == (None,) * 5


# ---- GPU ----

def plant_nonfinite(vis):
    """NaN / Inf at the first and last column, either side of a lane's and of a strip's edge."""
    nchan = vis.shape[-1]
    cols = sorted({c for c in (0, nchan - 1, V - 1, V, SW - 1, SW, 2 * SW - 1, 2 * SW, WPB * SW - 1, WPB * SW)
                   if 0 <= c < nchan})
    bad = [np.nan, np.inf, -np.inf]
    for k, c in enumerate(cols):
        t = k % vis.shape[2]
        vis[k % vis.shape[0], k % vis.shape[1], t, c] = bad[k % 3] if vis.dtype == np.float32 else \
            (complex(bad[k % 3], 1.0) if k % 2 else complex(1.0, bad[k % 3]))
    return vis


DYADIC_SHAPES = [(1, 1, 1, 1), (1, 1, 1, 2), (2, 1, 3, 255), (2, 1, 3, 256), (2, 1, 3, 257),
                 (1, 2, 2, V - 1), (1, 2, 2, V + 1), (2, 1, 3, SW - 1), (2, 1, 3, SW + 1),
                 (3, 2, 65, 513), (5, 4, 7, 1025), (1, 1, NT + ROWS + 1, 6), (1, 1, 5, WPB * SW + V)]
DYADIC_SHAPES = list(dict.fromkeys(DYADIC_SHAPES))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("shape", DYADIC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gpu_dyadic_inputs_bit_for_bit(gpu, shape, dtype):
    vis = plant_nonfinite(dyadic(shape, sum(shape), dtype))
    rnd = random_flags(shape, 11 + sum(shape))
    for flags in (rnd, rnd.astype(np.uint8) * 3, np.ones(shape, bool), np.zeros(shape, np.uint8)):
        got = quality.window_quality(vis, flags)
        assert isinstance(got, QualityStatistics) and got.shape == shape
        same_bits(got, restate_quality(vis, flags))


@pytest.mark.gpu
def test_gpu_both_load_routes_run_and_agree(gpu):
    """Sixteen-byte loads when the channel count and the bases allow them, scalar loads otherwise: the same bits."""
    import torch
    from tricolour_amd import _lib
    shape = (2, 2, 5, 2 * SW)
    for dtype, code in (("c64", 0), ("f32", 1)):
        vis, flags = plant_nonfinite(dyadic(shape, 21, dtype)), random_flags(shape, 22)
        want = restate_quality(vis, flags)
        n = int(np.prod(shape))
        for offset, vec in ((0, "true"), (1, "false")):
            v = torch.empty(n + 4, dtype=torch.from_numpy(vis).dtype, device="cuda")[offset:offset + n].view(shape)
            f = torch.empty(n + 4, dtype=torch.uint8, device="cuda")[offset:offset + n].view(shape)
            v.copy_(torch.from_numpy(vis))
            f.copy_(torch.from_numpy(flags.view(np.uint8)))
            _lib.kernel_log_begin()
            try:
                got = quality.window_quality(v, f)
            finally:
                log = _lib.kernel_log_end()
            same_bits(got, want)
            assert {k for k in log if k.startswith("k_quality_walk")} == {"k_quality_walk<%d, %s>" % (code, vec)}, log
            assert log.get("k_quality_window") == 1 and log.get("k_quality_fold") == 2, log


GAUSS_SHAPE = (5, 2, 67, 1025)


@pytest.mark.gpu
def test_gpu_gaussian_inputs_within_the_derived_bound(gpu):
    """Counts exact; every sum within 2 * (m + 8) * 2^-53 * S of the restatement (m terms, S the sum of their absolute
    values): at most 4 roundings per term on either side and m - 1 in the device's summation, unit roundoff 2^-53."""
    vis, flags = gaussian(GAUSS_SHAPE, 31), random_flags(GAUSS_SHAPE, 32)
    got = quality.window_quality(vis, flags)
    exact, absolute = restate_quality(vis, flags), restate_quality(vis, flags, absolute=True)
    ok, re_, im_, p, pair, dp = sample_terms(vis, flags)
    largest = 0.0
    for axis in quality.AXES:
        g, e, a = getattr(got, axis), getattr(exact, axis), getattr(absolute, axis)
        assert np.array_equal(g.n, e.n) and np.array_equal(g.dn, e.dn) and g.n.dtype == np.int64
        for name in SUMS:
            m = e.dn if name == "dsum_p" else e.n
            bound = 2.0 * (m + 8) * 2.0 ** -53 * getattr(a, name)
            err = np.abs(getattr(g, name) - getattr(e, name))
            print(axis, name, "largest error %.3g, its bound %.3g, largest bound %.3g"
                  % (err.max(), bound.flat[err.argmax()], bound.max()))
            assert (err <= bound).all(), (axis, name, float(err.max()))
            largest = max(largest, float(bound.max()))
    # A dropped or doubled sample cannot hide.  Every sample and every pair is a term of exactly one chan cell, and there
    # the smallest term kept is far above the largest bound (6e-11 against 5.6e-7 for this input).  The same does not
    # hold against the bl cells' bounds -- 55 000 terms each, up to 1.7e-6, above the smallest of 690 000 Gaussian draws
    # whatever the device does -- so the chan cells carry this check, besides the exact counts.
    smallest = min(np.abs(re_[ok]).min(), np.abs(im_[ok]).min(), p[ok].min(), dp[pair].min())
    e, a = exact.chan, absolute.chan
    largest_chan = max(float((2.0 * ((e.dn if name == "dsum_p" else e.n) + 8) * 2.0 ** -53 * getattr(a, name)).max())
                       for name in SUMS)
    print("smallest |term| %.3g, largest bound of a chan cell %.3g, of any cell %.3g" % (smallest, largest_chan, largest))
    assert smallest > 1000 * largest_chan


@pytest.mark.gpu
def test_gpu_order_contract(gpu, monkeypatch):
    """The same bits from run to run, for every batch of baselines, across calls continued with accumulate, and under a
    workspace budget that halves the batch."""
    import torch
    from tricolour_amd import _lib
    shape = (5, 2, 9, 300)
    vis, flags = gaussian(shape, 41), random_flags(shape, 42)
    one = quality.window_quality(vis, flags)
    same_bits(quality.window_quality(vis, flags), one)
    for b in (1, 2):
        same_bits(quality.window_quality(vis, flags, _max_baselines=b), one)
    # one call per baseline range through the Python layer
    head = quality.window_quality(vis[:3], flags[:3])
    same_bits(quality.window_quality(vis[3:], flags[3:], accumulate_into=head), one)
    # two ABI calls over baselines [0, 3) and [3, 5) with accumulate
    lib = _lib.lib()
    nbl, ncorr, ntime, nchan = shape
    v, f = torch.from_numpy(vis).cuda(), torch.from_numpy(flags.view(np.uint8)).cuda()
    nbytes = lib.tri_quality_workspace_bytes(3, ncorr, ntime, nchan)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ct, st = (torch.full((k, ncorr * ntime), 7, dtype=dt, device="cuda") for k, dt in ((2, torch.int64), (4, torch.float64)))
    cc, sc = (torch.full((k, ncorr * nchan), 7, dtype=dt, device="cuda") for k, dt in ((2, torch.int64), (4, torch.float64)))
    cells = []
    stream = torch.cuda.current_stream().cuda_stream
    for b0, b1 in ((0, 3), (3, 5)):
        cb = torch.empty((2, (b1 - b0) * ncorr), dtype=torch.int64, device="cuda")
        sb = torch.empty((4, (b1 - b0) * ncorr), dtype=torch.float64, device="cuda")
        _lib.check(lib.tri_window_quality(v[b0:].data_ptr(), _lib.TRI_VIS_C64, f[b0:].data_ptr(), b1 - b0, ncorr, ntime, nchan,
                                          cb.data_ptr(), sb.data_ptr(), ct.data_ptr(), st.data_ptr(), cc.data_ptr(),
                                          sc.data_ptr(), 1 if b0 else 0, ws.data_ptr(), ws.numel(), stream))
        cells.append((cb.cpu().numpy().reshape(2, b1 - b0, ncorr), sb.cpu().numpy().reshape(4, b1 - b0, ncorr)))
    assert np.array_equal(np.concatenate([c[0][0] for c in cells]), one.bl.n)
    assert np.array_equal(np.concatenate([c[1][3] for c in cells]), one.bl.dsum_p)
    assert np.array_equal(np.concatenate([c[1][0] for c in cells]), one.bl.sum_re)
    for got, want in ((ct, (one.time.n, one.time.dn)), (st, [getattr(one.time, k) for k in SUMS]),
                      (cc, (one.chan.n, one.chan.dn)), (sc, [getattr(one.chan, k) for k in SUMS])):
        assert np.array_equal(got.cpu().numpy(), np.stack([w.reshape(-1) for w in want]))
    # an empty call writes zeros, or leaves the accumulated cells alone, without a launch
    _lib.kernel_log_begin()
    try:
        for acc in (1, 0):
            _lib.check(lib.tri_window_quality(v.data_ptr(), _lib.TRI_VIS_C64, f.data_ptr(), 0, ncorr, ntime, nchan,
                                              cb.data_ptr(), sb.data_ptr(), ct.data_ptr(), st.data_ptr(),
                                              cc.data_ptr(), sc.data_ptr(), acc, None, 0, stream))
            assert bool(st.any()) == bool(acc) and bool(cc.any()) == bool(acc)
    finally:
        assert not _lib.kernel_log_end()
    # a budget under which the batch of 5 baselines halves to 3
    ws_bytes = lambda b: lib.tri_quality_workspace_bytes(b, ncorr, ntime, nchan)
    assert ws_bytes(3) + 64 < ws_bytes(5)
    monkeypatch.setenv("TRICOLOUR_AMD_WORKSPACE_GB", "%.15g" % ((ws_bytes(3) + 64) / float(1 << 30)))
    _lib.kernel_log_begin()
    try:
        halved = quality.window_quality(v, f)
    finally:
        log = _lib.kernel_log_end()
    assert log.get("k_quality_window") == 2, log
    same_bits(halved, one)


def quality_scan(seed):
    """6 baselines of 3 antennas, the autos among them, 5 times, 64 channels, 2 correlations."""
    rs = np.random.RandomState(seed)
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    ntime, nchan, ncorr = 5, 64, 2
    ant1 = np.array([p for _ in range(ntime) for p, _q in pairs], np.int32)
    ant2 = np.array([q for _ in range(ntime) for _p, q in pairs], np.int32)
    tm = np.repeat(4.0e9 + 8.0 * np.arange(ntime), len(pairs))
    nrow = tm.size
    data = (rs.standard_normal((nrow, nchan, ncorr)) + 1j * rs.standard_normal((nrow, nchan, ncorr))).astype(np.complex64)
    data[:, 20:22, :] *= np.float32(9)
    data[7, 40, 1] = np.nan
    flags = rs.random_sample(data.shape) < 0.05
    return data, flags, ant1, ant2, tm, np.linspace(1.0e9, 1.1e9, nchan), np.full(nchan, 1.0e8 / nchan)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["standard", "total_power"])
def test_gpu_flag_scan_fills_the_quality_of_the_packed_windows(gpu, mode):
    from tricolour_amd import _lib, packing, scan
    from tricolour_amd.strategies import apply_strategies
    from test_scan_gpu import _plain
    data, flags, ant1, ant2, tm, freq, width = quality_scan(51)
    strategies = [{"task": "flag_autos"},
                  {"task": "sum_threshold", "kwargs": dict(num_major_iterations=1, background_iterations=1)}]
    kw = dict(flagging_strategy=mode, corr_type=[9, 12])
    _lib.kernel_log_begin()
    try:
        plain = scan.flag_scan(data, flags, ant1, ant2, tm, freq, width, strategies, **kw)
    finally:
        log = _lib.kernel_log_end()
    assert len(plain) == 3 and not [k for k in log if k.startswith("k_quality")], log
    q = quality.ScanQuality()
    whole = scan.flag_scan(data, flags, ant1, ant2, tm, freq, width, strategies, quality=q, **kw)
    assert len(whole) == 3 and np.array_equal(whole[0], plain[0])
    assert _plain(whole[1]) == _plain(plain[1]) and _plain(whole[2]) == _plain(plain[2])

    ubl = packing.unique_baselines(ant1, ant2)
    utime, time_inv = np.unique(tm, return_inverse=True)
    vis_w, flag_w = packing.pack_scan(time_inv.astype(np.int32), ubl, ant1, ant2, data, flags, utime.size,
                                      flagging_strategy=mode, stokes_terms=scan._stokes_terms(mode, [9, 12]))
    assert tuple(vis_w.shape) == (6, 2 if mode == "standard" else 1, 5, 64)
    after = apply_strategies(strategies, flag_w, vis_w, ubl=ubl, ant_pos=None, chan_freq=freq, chan_width=width,
                             masked_channels=[])
    want_original, want_final = quality.window_quality(vis_w, flag_w), quality.window_quality(vis_w, after)
    same_bits(q.original, want_original)
    same_bits(q.final, want_final)
    assert (q.final.bl.n <= q.original.bl.n).all() and (q.final.bl.n < q.original.bl.n).any()
    autos = ubl[:, 1] == ubl[:, 2]
    assert autos.sum() == 3 and not q.final.bl.n[autos].any() and q.original.bl.n[autos].all() and q.final.bl.n[~autos].all()
    assert np.array_equal(q.ubl, ubl) and np.array_equal(q.chan_freq, freq) and np.array_equal(q.times, utime)

    qc = quality.ScanQuality()
    chunked = scan.flag_scan(data, flags, ant1, ant2, tm, freq, width, strategies, quality=qc, baseline_chunks=2, **kw)
    assert np.array_equal(chunked[0], plain[0])
    same_bits(qc.original, q.original)
    same_bits(qc.final, q.final)
    assert np.array_equal(qc.ubl, ubl)

    ds = dict(DATA=data, FLAG=flags, ANTENNA1=ant1, ANTENNA2=ant2, TIME=tm, CHAN_FREQ=freq, CHAN_WIDTH=width,
              FIELD_ID=0, DATA_DESC_ID=0, SCAN_NUMBER=1, CORR_TYPE=[9, 12])
    got = []
    out, summary = scan.flag_scans([ds, dict(ds, SCAN_NUMBER=2)], strategies, scan_numbers=[1], flagging_strategy=mode,
                                   quality=got)
    assert out[1] is None and len(got) == 1 and isinstance(got[0], quality.ScanQuality)
    same_bits(got[0].final, q.final)
    assert quality.summarise_quality(got[0].final, got[0].original)[3] == "Per correlation, over channels:"
