"""Sliding-window complex deviation thresholding (``threshold_local_deviation``):
the NumPy restatement of the definition (``include/tricolour_amd.h``) against a
plain per-sample loop, its properties, its behaviour on noise and on a
phase-scrambled fringe and the strategy plumbing on the CPU; the device kernels
against the restatement on the GPU.

No tolerance anywhere.  Every arithmetic step of the definition is a correctly
rounded IEEE operation in a fixed order (float64 adds, products, divisions and
one square root, one narrowing cast, float32 for the even median), on both
sides, so the deviation images must agree in every bit, NaN positions
included, and the flags must be equal.  A difference means the order of a sum
is wrong, a multiply-add was contracted or a median picked the wrong element.

This module also keeps the kernel table of ``tricolour_amd/csrc/steps/ldev/``:
KERNELS lists every ``__global__`` kernel there with each instantiation a
launch site can produce; a CPU test holds it to the sources, and the last GPU
test shows with the library's kernel log that every listed instantiation was
launched by a call whose result was compared with the restatement."""
import contextlib
import glob
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT

TASK = "threshold_local_deviation"
DEFAULTS = dict(window_time=3, window_freq=3, scale_time=3.5, scale_freq=3.5, freq_chunks=10)
NAN32 = np.uint32(0x7FC00000).view(np.float32)

# every __global__ kernel of csrc/steps/ldev/ and its instantiations, in the spelling of the kernel log
# (k_ldev_time / k_ldev_freq <VIS, W, VEC>: VIS 0 = complex64, 1 = float32 amplitudes; W 3, 5 or 0 = any other width)
KERNELS = {
    "k_ldev_time": {"k_ldev_time<%d, %d, %s>" % (v, w, b) for v in (0, 1) for w in (3, 5, 0) for b in ("true", "false")},
    "k_ldev_freq": {"k_ldev_freq<%d, %d, %s>" % (v, w, b) for v in (0, 1) for w in (3, 5, 0) for b in ("true", "false")},
    "k_ldev_level": {"k_ldev_level<0>", "k_ldev_level<1>"},
    "k_ldev_apply": {"k_ldev_apply<true>", "k_ldev_apply<false>"},
}
MET = set()        # instantiations launched by calls whose results equalled the restatement


# ---------------------------------------------------------------------------
# the definition, restated (vectorised) ...
# ---------------------------------------------------------------------------
def parts(vis):
    vis = np.asarray(vis)
    if np.iscomplexobj(vis):
        return vis.real.astype(np.float32), vis.imag.astype(np.float32)
    return vis.astype(np.float32), np.zeros(vis.shape, np.float32)


def _shift(a, o, fill):
    """b[..., i] = a[..., i + o], `fill` beyond the ends."""
    n = a.shape[-1]
    b = np.full(a.shape, fill, a.dtype)
    if o >= 0:
        if o < n:
            b[..., :n - o] = a[..., o:]
    elif -o < n:
        b[..., -o:] = a[..., :n + o]
    return b


def _deviation_last_axis(re, im, counts, window):
    """d along the last axis: float32, NaN where unusable, +inf where the window holds a counting infinite part."""
    h = (window - 1) // 2
    re64, im64 = re.astype(np.float64), im.astype(np.float64)
    inf = counts & (np.isinf(re) | np.isinf(im))
    n = np.zeros(re.shape, np.int64)
    sr, si = np.zeros(re.shape), np.zeros(re.shape)
    anyinf = np.zeros(re.shape, bool)
    with np.errstate(all="ignore"):
        for o in range(-h, h + 1):                              # ascending position
            c = _shift(counts, o, False)
            n += c
            sr = np.where(c, sr + _shift(re64, o, 0.0), sr)
            si = np.where(c, si + _shift(im64, o, 0.0), si)
            anyinf |= _shift(inf, o, False)
        nn = n.astype(np.float64)
        mr, mi = sr / nn, si / nn
        acc = np.zeros(re.shape)
        for o in range(-h, h + 1):
            c = _shift(counts, o, False)
            dr = _shift(re64, o, 0.0) - mr
            acc = np.where(c, acc + dr * dr, acc)
            di = _shift(im64, o, 0.0) - mi
            acc = np.where(c, acc + di * di, acc)
        d = np.sqrt(acc / nn).astype(np.float32)
    usable = counts & (n >= 2)
    d[usable & anyinf] = np.inf
    d[~usable] = NAN32
    return d


def restate_deviation(vis, flags, window_time=3, window_freq=3):
    """(d_time, d_freq) of (..., time, chan) inputs."""
    re, im = parts(vis)
    counts = (np.asarray(flags) == 0) & ~np.isnan(re) & ~np.isnan(im)
    sw = lambda a: np.swapaxes(a, -1, -2)
    d_t = sw(_deviation_last_axis(sw(re), sw(im), sw(counts), window_time))
    d_f = _deviation_last_axis(re, im, counts, window_freq)
    return np.ascontiguousarray(d_t), np.ascontiguousarray(d_f)


def _hits_last_axis(d, scale):
    """Lines along the last axis: level = median of the finite d; the hits."""
    fin = np.isfinite(d)
    m = fin.sum(axis=-1, keepdims=True)
    s = np.sort(np.where(fin, d, np.float32(np.inf)), axis=-1)
    top = d.shape[-1] - 1
    a = np.take_along_axis(s, np.clip((m - 1) // 2, 0, top), axis=-1)
    b = np.take_along_axis(s, np.clip(m // 2, 0, top), axis=-1)
    with np.errstate(all="ignore"):
        med = np.where(m % 2 == 1, a, (a + b).astype(np.float32) / np.float32(2)).astype(np.float32)
        live = (m >= 3) & (med > 0)
        over = d.astype(np.float64) > med.astype(np.float64) * np.float64(scale)
    return ~np.isnan(d) & (np.isposinf(d) | (live & over))


def chunk_ends(nchan, freq_chunks):
    return np.linspace(0, nchan, freq_chunks + 1).astype(int)


def restate_threshold(vis, flags, window_time=3, window_freq=3, scale_time=3.5, scale_freq=3.5, freq_chunks=10, dev=None):
    f = np.asarray(flags) != 0
    d_t, d_f = dev if dev is not None else restate_deviation(vis, flags, window_time, window_freq)
    out = f.copy()
    if scale_time > 0 and d_t.size:
        out |= np.swapaxes(_hits_last_axis(np.swapaxes(d_t, -1, -2), scale_time), -1, -2)
    if scale_freq > 0 and d_f.size:
        ends = chunk_ends(f.shape[-1], freq_chunks)
        for lo, hi in zip(ends[:-1], ends[1:]):
            if hi > lo:
                out[..., lo:hi] |= _hits_last_axis(d_f[..., lo:hi], scale_freq)
    return out


# ---------------------------------------------------------------------------
# ... and as a plain per-sample loop over one (time, chan) window
# ---------------------------------------------------------------------------
def loop_deviation(vis, flags, window, axis):
    T, F = vis.shape
    re, im = parts(vis)
    h = (window - 1) // 2
    d = np.empty((T, F), np.float32)
    for t in range(T):
        for c in range(F):
            if axis == 0:
                slots = [(tt, c) for tt in range(max(0, t - h), min(T - 1, t + h) + 1)]
            else:
                slots = [(t, cc) for cc in range(max(0, c - h), min(F - 1, c + h) + 1)]
            cnt = [p for p in slots if not flags[p] and not math.isnan(re[p]) and not math.isnan(im[p])]
            n, sr, si = len(cnt), 0.0, 0.0
            for p in cnt:
                sr += float(re[p])
                si += float(im[p])
            if (t, c) not in cnt or n < 2:
                d[t, c] = NAN32
                continue
            if any(math.isinf(re[p]) or math.isinf(im[p]) for p in cnt):
                d[t, c] = np.inf
                continue
            mr, mi, acc = sr / float(n), si / float(n), 0.0
            for p in cnt:
                dr, di = float(re[p]) - mr, float(im[p]) - mi
                acc = acc + dr * dr
                acc = acc + di * di
            with np.errstate(over="ignore"):
                d[t, c] = np.float32(math.sqrt(acc / float(n)))
    return d


def loop_hits(line, scale):
    vals = sorted(np.float32(x) for x in line if np.isfinite(x))
    m = len(vals)
    live, med = False, np.float32(0)
    if m:
        with np.errstate(over="ignore"):
            med = vals[(m - 1) // 2] if m % 2 else np.float32(vals[m // 2 - 1] + vals[m // 2]) / np.float32(2)
        live = m >= 3 and med > 0
    return [(not np.isnan(x)) and (x == np.inf or (live and float(x) > float(med) * scale)) for x in line]


def loop_threshold(vis, flags, window_time=3, window_freq=3, scale_time=3.5, scale_freq=3.5, freq_chunks=10):
    T, F = vis.shape
    out = np.asarray(flags) != 0
    out = out.copy()
    d_t, d_f = loop_deviation(vis, flags, window_time, 0), loop_deviation(vis, flags, window_freq, 1)
    if scale_time > 0:
        for c in range(F):
            out[:, c] |= np.array(loop_hits(d_t[:, c], scale_time), bool)
    if scale_freq > 0:
        ends = chunk_ends(F, freq_chunks)
        for t in range(T):
            for lo, hi in zip(ends[:-1], ends[1:]):
                if hi > lo:
                    out[t, lo:hi] |= np.array(loop_hits(d_f[t, lo:hi], scale_freq), bool)
    return d_t, d_f, out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    view = {8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize]
    return np.array_equal(a.view(view), b.view(view))


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def make_case(shape, seed, density=0.05, dtype="c64", special=False):
    """Noise whose level varies over 6 decades from channel to channel (so that sums round and medians differ from line
    to line), some strong outliers, `density` input flags; special: unflagged NaN and infinite samples."""
    rng = np.random.default_rng(seed)
    if dtype == "c64":
        vis = np.empty(shape, np.complex64)
        vis.real = rng.standard_normal(shape, dtype=np.float32)
        vis.imag = rng.standard_normal(shape, dtype=np.float32)
    else:
        vis = rng.standard_normal(shape, dtype=np.float32)
    vis *= (10.0 ** rng.uniform(-3.0, 3.0, size=(shape[0], 1, 1, shape[3]))).astype(np.float32)
    vis[rng.uniform(size=shape) < 0.03] *= np.float32(30)
    flags = rng.uniform(size=shape) < density
    if special and vis.size:
        flat = vis.reshape(-1)
        fl = flags.reshape(-1)
        pos = rng.choice(flat.size, size=min(flat.size, 8), replace=False)
        if dtype == "c64":
            values = [complex(np.nan, 1.0), complex(1.0, np.nan), complex(np.inf, 2.0), complex(2.0, -np.inf),
                      complex(np.inf, np.nan), complex(np.nan, np.nan), complex(-np.inf, np.inf), complex(np.inf, 1.0)]
        else:
            values = [np.nan, np.nan, np.inf, -np.inf, np.inf, np.nan, -np.inf, np.inf]
        for p, v in zip(pos, values):
            flat[p] = v
            fl[p] = False
        if flat.size > 8:                                       # ... and a flagged infinite sample, which must not be seen
            q = int(pos[0] + 1) % flat.size
            if q not in pos:
                flat[q] = np.inf
                fl[q] = True
    return vis, flags


_CACHE = {}


def expected(key, vis, flags, kw):
    """(d_time, d_freq, out) of the restatement; computed once per key and left unchanged."""
    if key not in _CACHE:
        dev = restate_deviation(vis, flags, kw.get("window_time", 3), kw.get("window_freq", 3))
        _CACHE[key] = dev + (restate_threshold(vis, flags, dev=dev, **kw),)
    return _CACHE[key]


def noise_input(seed=1, shape=(128, 192)):
    rng = np.random.default_rng(seed)
    vis = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    flags = rng.uniform(size=shape) < 0.02
    return vis, flags


def scrambled_patch_input():
    """Unit complex noise plus a constant-amplitude 20 sigma fringe; in 6 times x 3 channels the fringe's phase is
    scrambled (its amplitude is not), 2 % input flags."""
    rng = np.random.default_rng(3)
    shape = (128, 192)
    noise = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    t, c = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    phase = 2 * np.pi * (0.003 * t + 0.002 * c)
    patch = np.zeros(shape, bool)
    patch[60:66, 90:93] = True
    phase = np.where(patch, rng.uniform(0, 2 * np.pi, size=shape), phase)
    vis = (noise + 20.0 * np.exp(1j * phase)).astype(np.complex64)
    flags = rng.uniform(size=shape) < 0.02
    flags[patch] = False
    return vis, flags, patch


def dilate(mask, h):
    out = mask.copy()
    for o in range(1, h + 1):
        out[o:] |= mask[:-o]
        out[:-o] |= mask[o:]
        out[:, o:] |= mask[:, :-o]
        out[:, :-o] |= mask[:, o:]
    return out


# ---------------------------------------------------------------------------
# CPU: the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["c64", "f32"])
def test_restatement_equals_the_per_sample_loop(dtype):
    cases = [((1, 1, 7, 9), dict(DEFAULTS, freq_chunks=2), False), ((1, 1, 6, 5), dict(DEFAULTS, window_time=5, window_freq=9), True),
             ((1, 1, 1, 8), dict(DEFAULTS, freq_chunks=3), False), ((1, 1, 9, 1), DEFAULTS, False),
             ((1, 1, 12, 10), dict(window_time=5, window_freq=3, scale_time=1.5, scale_freq=1.2, freq_chunks=13), True),
             ((1, 1, 8, 12), dict(DEFAULTS, scale_time=0.0, scale_freq=1.1, freq_chunks=4), True),
             ((1, 1, 10, 6), dict(DEFAULTS, scale_time=1.1, scale_freq=0.0), False)]
    for i, (shape, kw, special) in enumerate(cases):
        vis, flags = make_case(shape, 10 + i, 0.15, dtype, special)
        vis[0, 0, :, 0] = vis[0, 0, 0, 0]                       # a line of identical values: level 0
        d_t, d_f = restate_deviation(vis, flags, kw["window_time"], kw["window_freq"])
        out = restate_threshold(vis, flags, **kw)
        l_t, l_f, l_out = loop_threshold(vis[0, 0], flags[0, 0], **kw)
        assert same_bits(d_t[0, 0], l_t) and same_bits(d_f[0, 0], l_f), (shape, kw)
        assert np.array_equal(out[0, 0], l_out), (shape, kw)


def test_restatement_properties():
    kw = dict(DEFAULTS, scale_time=1.5, scale_freq=1.5, freq_chunks=3)
    vis, flags = make_case((3, 2, 20, 31), 20, 0.1, "c64", True)
    out = restate_threshold(vis, flags, **kw)
    assert (out >= flags).all() and (out & ~flags).any() and not out.all()              # out contains f
    assert np.array_equal(restate_threshold(vis, flags, **dict(kw, scale_time=0.0, scale_freq=0.0)), flags)
    full = np.ones(flags.shape, bool)
    assert np.array_equal(restate_threshold(vis, full, **kw), full)                     # all flagged: nothing to add
    one = flags.copy()
    one[1, 1] = True                                                                   # one all-flagged window
    assert restate_threshold(vis, one, **kw)[1, 1].all()
    assert np.isnan(restate_deviation(vis, one)[0][1, 1]).all()
    # a stack of windows equals the windows one by one
    for b in range(3):
        for p in range(2):
            assert np.array_equal(out[b, p], restate_threshold(vis[b:b + 1, p:p + 1], flags[b:b + 1, p:p + 1], **kw)[0, 0])
    # either axis alone gives a subset, both give the union
    t_only = restate_threshold(vis, flags, **dict(kw, scale_freq=0.0))
    f_only = restate_threshold(vis, flags, **dict(kw, scale_time=0.0))
    assert np.array_equal(out, t_only | f_only) and (t_only != f_only).any()


def test_restatement_float32_input_is_complex_input_with_zero_imaginary_part():
    amp, flags = make_case((2, 1, 15, 22), 21, 0.1, "f32", True)
    as_c = amp.astype(np.complex64)
    assert not as_c.imag.any()
    for a, b in zip(restate_deviation(amp, flags, 5, 3), restate_deviation(as_c, flags, 5, 3)):
        assert same_bits(a, b)
    kw = dict(DEFAULTS, scale_time=1.5, scale_freq=1.5, freq_chunks=2)
    assert np.array_equal(restate_threshold(amp, flags, **kw), restate_threshold(as_c, flags, **kw))


def test_restatement_single_row_or_channel_disables_that_axis():
    vis, flags = make_case((2, 1, 1, 40), 22, 0.1)
    d_t, d_f = restate_deviation(vis, flags)
    assert np.isnan(d_t).all() and np.isfinite(d_f).any()
    kw = dict(DEFAULTS, scale_time=0.1, scale_freq=1.5, freq_chunks=2)
    assert np.array_equal(restate_threshold(vis, flags, **kw), restate_threshold(vis, flags, **dict(kw, scale_time=0.0)))
    assert np.array_equal(restate_threshold(vis, flags, **dict(kw, scale_freq=0.0)), flags)    # T == 1: time flags nothing


def test_restatement_nonfinite_samples():
    vis = np.ones((1, 1, 9, 9), np.complex64) * np.arange(9, dtype=np.float32)[None, None, :, None]
    vis += (np.arange(9, dtype=np.float32) ** 2)[None, None, None, :]
    flags = np.zeros(vis.shape, bool)
    vis[0, 0, 4, 4] = complex(np.inf, 1.0)
    vis[0, 0, 2, 2] = complex(np.nan, 1.0)
    vis[0, 0, 6, 6] = complex(np.inf, np.nan)          # a NaN part: does not count, the infinite part is not seen
    vis[0, 0, 6, 2] = np.inf
    flags[0, 0, 6, 2] = True                            # flagged: not seen either
    d_t, d_f = restate_deviation(vis, flags)
    assert np.isposinf(d_t[0, 0, 3:6, 4]).all() and np.isposinf(d_f[0, 0, 4, 3:6]).all()
    assert np.isposinf(d_t).sum() == 3 and np.isposinf(d_f).sum() == 3
    assert np.isnan(d_t[0, 0, 2, 2]) and np.isnan(d_t[0, 0, 6, 6]) and np.isnan(d_t[0, 0, 6, 2])
    assert np.isnan(d_t).sum() == 3 and np.isfinite(d_t[0, 0, 5, 6]) and np.isfinite(d_t[0, 0, 7, 2])
    out = restate_threshold(vis, flags, scale_time=1e30, scale_freq=1e30)
    exp = flags.copy()
    exp[0, 0, 3:6, 4] = True
    exp[0, 0, 4, 3:6] = True
    assert np.array_equal(out, exp)                     # +inf is always a hit; NaN never is


def test_default_step_is_inert_on_noise():
    """Seeded unit complex Gaussian noise, 128 x 192, 2 % pre-flagged, the default kwargs: no flag is added."""
    vis, flags = noise_input(seed=1)
    out = restate_threshold(vis[None, None], flags[None, None], **DEFAULTS)[0, 0]
    assert 0.015 < flags.mean() < 0.025
    assert np.array_equal(out, flags), int((out & ~flags).sum())


def test_behaviour_phase_scrambled_patch():
    """The amplitude inside the patch is that of the fringe everywhere else; the step finds every cell of the patch and
    flags nothing outside the patch dilated by h along each axis."""
    vis, flags, patch = scrambled_patch_input()
    amp = np.abs(vis)
    assert abs(amp[patch].mean() / amp[~patch].mean() - 1.0) < 0.02
    out = restate_threshold(vis[None, None], flags[None, None], **DEFAULTS)[0, 0]
    new = out & ~flags
    assert patch.sum() == 18 and new[patch].all()
    assert not (new & ~dilate(patch, 1)).any(), int((new & ~dilate(patch, 1)).sum())


# ---------------------------------------------------------------------------
# CPU: plumbing
# ---------------------------------------------------------------------------
def test_the_task_is_valid_and_checked():
    from tricolour_amd import scan
    assert TASK in scan.VALID_TASKS and TASK not in scan.WHOLE_SCAN_TASKS
    scan.check_strategies([{"task": TASK}, {"task": TASK, "kwargs": dict(DEFAULTS)}, {"task": TASK, "kwargs": None},
                           {"task": TASK, "kwargs": dict(window_time=31, window_freq=5, scale_time=0, scale_freq=0.0,
                                                         freq_chunks=1)}])
    bad = [dict(window_time=4), dict(window_freq=2), dict(window_time=1), dict(window_freq=33), dict(window_time=-3),
           dict(window_time=3.5), dict(window_freq="3"), dict(scale_time=-0.1), dict(scale_freq=-1),
           dict(scale_time=float("nan")), dict(scale_freq=float("nan")), dict(scale_time=None), dict(freq_chunks=0),
           dict(freq_chunks=-2), dict(freq_chunks=2.5), dict(window=3)]
    for kw in bad:
        with pytest.raises(ValueError, match=TASK):
            scan.check_strategies([{"task": "flag_autos"}, {"task": TASK, "kwargs": kw}])


def test_python_argument_errors_come_before_any_device_work():
    from tricolour_amd import flagging
    vis = np.zeros((3, 1, 4, 8), np.complex64)
    flags = np.zeros((3, 1, 4, 8), bool)
    for fn in (flagging.local_deviation, flagging.threshold_local_deviation):
        with pytest.raises(ValueError):
            fn(vis, flags[:, :, :3])
        with pytest.raises(ValueError):
            fn(vis[0], flags[0])
        for kw in (dict(window_time=4), dict(window_freq=33), dict(window_time=1)):
            with pytest.raises(ValueError, match="window"):
                fn(vis, flags, **kw)
    for kw in (dict(scale_time=-1.0), dict(scale_freq=float("nan")), dict(freq_chunks=0)):
        with pytest.raises(ValueError):
            flagging.threshold_local_deviation(vis, flags, **kw)


def test_header_declares_and_the_binding_exports_the_entry_points():
    from tricolour_amd import _lib
    with open(os.path.join(ROOT, "include", "tricolour_amd.h")) as fh:
        hdr = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name, res in (("tri_local_deviation_workspace_bytes", "size_t"), ("tri_local_deviation", "int"),
                      ("tri_local_deviation_threshold", "int")):
        assert re.search(r"\b%s\s+%s\s*\(" % (res, name), hdr), name
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().tri_version() >= 104
    assert os.path.join(ROOT, "tricolour_amd", "csrc", "steps", "ldev", "kernels_ldev.hpp") in _lib.DEPENDS


def test_abi_rejects_bad_arguments_without_a_launch():
    import ctypes as C
    from tricolour_amd import _lib
    lib = _lib.lib()
    buf = (C.c_uint8 * 16384)()
    base = C.addressof(buf)
    v, f, o, d = base, base + 4096, base + 8192, base + 12288
    ends = (C.c_int64 * 3)(0, 4, 8)

    def dev(vis=v, dtype=_lib.TRI_VIS_C64, flags=f, n_win=2, ntime=4, nchan=8, wt=3, wf=3, dt=d, df=d):
        return lib.tri_local_deviation(vis, dtype, flags, n_win, ntime, nchan, wt, wf, dt, df, None)

    def thr(vis=v, dtype=_lib.TRI_VIS_C64, flags=f, out=o, n_win=2, ntime=4, nchan=8, wt=3, wf=3, st=3.5, sf=3.5,
            ce=ends, nce=3, ws=d, wsb=0):
        return lib.tri_local_deviation_threshold(vis, dtype, flags, out, n_win, ntime, nchan, wt, wf, st, sf, ce, nce,
                                                 ws, wsb, None)
    for kw in (dict(vis=None), dict(flags=None), dict(n_win=-1), dict(ntime=-1), dict(nchan=-1), dict(wt=4), dict(wf=1),
               dict(wt=33), dict(wf=-3)):
        assert dev(**kw) == _lib.TRI_EINVAL, kw
        assert thr(**kw) == _lib.TRI_EINVAL, kw
    for kw in (dict(out=None), dict(ce=None), dict(st=-1.0), dict(sf=float("nan")), dict(nce=1), dict(nchan=9),
               dict(ce=(C.c_int64 * 3)(0, 5, 4)), dict(ce=(C.c_int64 * 3)(1, 4, 8)), dict(out=f + 8)):
        assert thr(**kw) == _lib.TRI_EINVAL, kw
    for dt in (_lib.TRI_VIS_C128, _lib.TRI_VIS_F64, 17, -1):
        assert dev(dtype=dt) == _lib.TRI_EUNSUPPORTED and thr(dtype=dt) == _lib.TRI_EUNSUPPORTED
    assert dev(n_win=0) == _lib.TRI_OK and dev(ntime=0) == _lib.TRI_OK               # empty: no launch
    assert thr(n_win=0) == _lib.TRI_OK and thr(ntime=0) == _lib.TRI_OK
    assert thr(nchan=0, ce=(C.c_int64 * 2)(0, 0), nce=2) == _lib.TRI_OK
    assert thr() == _lib.TRI_EWORKSPACE and thr(ws=None, wsb=1 << 30) == _lib.TRI_EWORKSPACE
    need = lib.tri_local_deviation_workspace_bytes(2, 4, 8, 3)
    assert need >= 2 * 4 * 8 * 10 + 24 and thr(wsb=need - 1) == _lib.TRI_EWORKSPACE
    assert lib.tri_local_deviation_workspace_bytes(0, 4, 8, 3) == 0
    assert lib.tri_local_deviation_workspace_bytes(4, 4, 8, 3) > need


# ---------------------------------------------------------------------------
# CPU: the kernel table against the sources
# ---------------------------------------------------------------------------
def scan_ldev_kernels():
    found = set()
    paths = sorted(glob.glob(os.path.join(ROOT, "tricolour_amd", "csrc", "steps", "ldev", "*")))
    assert paths
    for path in paths:
        with open(path, encoding="utf-8") as fh:
            found.update(re.findall(r"__global__[\s\S]{0,200}?\b(k_\w+)\s*\(", fh.read()))
    return found


def test_kernel_table_lists_what_the_sources_hold():
    from test_route_ledger import scan_instances, scan_kernels
    assert scan_ldev_kernels() == set(KERNELS)
    assert not set(KERNELS) & scan_kernels()                   # the ledger keeps the kernels directly under csrc/
    sites = scan_instances()                                   # launch sites of the host code, macros expanded
    for kernel, instances in KERNELS.items():
        assert sites.get(kernel) == instances, kernel
    with open(os.path.join(ROOT, "tricolour_amd", "csrc", "tricolour_amd.hip"), encoding="utf-8") as fh:
        assert '#include "steps/ldev/kernels_ldev.hpp"' in fh.read()


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@contextlib.contextmanager
def compared():
    """Yields a dict that receives the kernel log of the block; the step's kernels launched inside count as met if
    the block's comparisons passed."""
    import torch
    from tricolour_amd import _lib
    log = {}
    _lib.kernel_log_begin()
    try:
        yield log
        torch.cuda.synchronize()
    except BaseException:
        _lib.kernel_log_end()
        raise
    log.update(_lib.kernel_log_end())
    MET.update(k for k in log if k.startswith("k_ldev_"))


def dev(torch, a, offset=False):
    """A device copy of `a`; offset: a contiguous view whose base lies one element past an aligned address."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        return t.cuda()
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    flat[1:] = t.reshape(-1).cuda()
    return flat[1:].view(t.shape)


def check(key, vis, flags, kw, container="tensor", offset=False, max_windows=None):
    """local_deviation and threshold_local_deviation on the device against the restatement: bits of both images, the
    flags, the result's container and dtype, and the inputs unchanged."""
    import torch
    from tricolour_amd import flagging
    e_t, e_f, e_out = expected(key, vis, flags, kw)
    wkw = dict(window_time=kw.get("window_time", 3), window_freq=kw.get("window_freq", 3))
    extra = {} if max_windows is None else dict(_max_windows=max_windows)
    if container == "numpy":
        v, f = vis.copy(), flags.copy()
    else:
        v, f = dev(torch, vis, offset), dev(torch, flags, offset)
        if offset and vis.size:
            assert v.data_ptr() % 16 != 0
        f0 = f.clone()
    d_t, d_f = flagging.local_deviation(v, f, **wkw, **extra)
    out = flagging.threshold_local_deviation(v, f, **kw, **extra)
    if container == "numpy":
        assert isinstance(d_t, np.ndarray) and isinstance(d_f, np.ndarray) and isinstance(out, np.ndarray)
        assert out.dtype == flags.dtype
        assert same_bits(v, vis) and np.array_equal(f, flags)
    else:
        assert d_t.is_cuda and d_f.is_cuda and out.is_cuda and out.dtype == f.dtype
        assert same_bits(v.cpu().numpy(), vis) and torch.equal(f, f0)
        d_t, d_f, out = d_t.cpu().numpy(), d_f.cpu().numpy(), out.cpu().numpy()
    assert d_t.dtype == np.float32 and d_f.dtype == np.float32 and d_t.shape == vis.shape and d_f.shape == vis.shape
    bad_t, bad_f = int((d_t.view(np.uint32) != e_t.view(np.uint32)).sum()), int((d_f.view(np.uint32) != e_f.view(np.uint32)).sum())
    assert bad_t == 0 and bad_f == 0, "%s: %d d_time and %d d_freq bit patterns differ" % (key, bad_t, bad_f)
    nbad = int(((out != 0) != e_out).sum())
    assert out.shape == e_out.shape and nbad == 0, "%s: %d flags differ" % (key, nbad)
    return e_t, e_f, e_out


SHAPES = [
    ((1, 1, 1, 40), {}), ((2, 1, 40, 1), {}), ((1, 1, 2, 3), {}),
    ((1, 1, 5, 7), dict(window_time=9, window_freq=9)),                       # windows wider than the lines
    ((3, 2, 67, 133), {}), ((3, 2, 67, 133), dict(window_time=5, window_freq=9)),
    ((3, 2, 67, 133), dict(window_time=31, window_freq=5)), ((3, 2, 67, 133), dict(window_time=9, window_freq=31)),
    ((2, 1, 130, 260), {}), ((2, 1, 130, 260), dict(window_time=5, window_freq=5)),
    # one row and one column beyond the tiles: 64 rows (time), 8 rows (frequency), 1024 channels, 32 channels (levels)
    ((1, 1, 65, 1025), dict(window_time=5, window_freq=3)), ((1, 2, 65, 1028), dict(window_time=3, window_freq=5)),
    ((1, 1, 9, 1028), dict(window_time=31, window_freq=9)),
]


def shape_id(p):
    return "x".join(map(str, p[0])) + "".join("-%s%s" % (k[7], v) for k, v in sorted(p[1].items()))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("case", SHAPES, ids=shape_id)
def test_gpu_shapes_and_windows(gpu, case, dtype):
    """Aligned (the 16-byte route where nchan % 4 == 0) and at a one-element offset (the scalar route), as tensors; the
    low scales make both axes flag a few per cent, so a wrong level shows."""
    shape, wkw = case
    kw = dict(DEFAULTS, scale_time=1.8, scale_freq=1.8, freq_chunks=3, **wkw)
    vis, flags = make_case(shape, 40 + sum(shape), 0.05, dtype)
    key = ("shape", shape_id(case), dtype)
    with compared():
        _, _, out = check(key, vis, flags, kw)
        check(key, vis, flags, kw, offset=True)
    if min(shape[2:]) >= 40:
        assert (out & ~flags).any() and not out.all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("container", ["numpy", "tensor"])
def test_gpu_containers(gpu, container, dtype):
    import torch
    from tricolour_amd import flagging
    vis, flags = make_case((2, 2, 33, 52), 60, 0.05, dtype, special=True)
    kw = dict(DEFAULTS, scale_time=1.8, scale_freq=1.8, freq_chunks=2)
    with compared():
        _, _, e_out = check(("containers", dtype), vis, flags, kw, container=container)
        if container == "tensor":                              # uint8 flags with any nonzero byte: uint8 0 / 1 comes back
            f3 = dev(torch, flags.astype(np.uint8) * 3)
            out = flagging.threshold_local_deviation(dev(torch, vis), f3, **kw)
            assert out.is_cuda and out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), e_out.astype(np.uint8))
            assert torch.equal(f3, dev(torch, flags.astype(np.uint8) * 3))
        else:
            out = flagging.threshold_local_deviation(vis, flags.astype(np.uint8) * 5, **kw)
            assert out.dtype == np.uint8 and np.array_equal(out, e_out.astype(np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
def test_gpu_levels(gpu, dtype):
    """freq_chunks 1, 4 and more than F (empty chunks, and chunks of one and two channels: fewer than 3 usable samples),
    a channel flagged throughout, a line of identical values (level 0), a row flagged throughout, each axis alone."""
    shape = (2, 1, 37, 50)
    vis, flags = make_case(shape, 70, 0.05, dtype)
    flags[:, :, :, 7] = True
    flags[:, :, 11, :] = True
    vis[0, 0, :, 20] = vis[0, 0, 0, 20]
    vis[1, 0, 5, :] = vis[1, 0, 5, 0]
    for chunks in (1, 4, 50, 120):
        for st, sf in ((1.8, 1.8), (1.8, 0.0), (0.0, 1.8), (0.0, 0.0)):
            kw = dict(DEFAULTS, scale_time=st, scale_freq=sf, freq_chunks=chunks)
            with compared():
                e_t, e_f, out = check(("levels", dtype, chunks, st, sf), vis, flags, kw)
            if st == 0.0 and sf == 0.0:
                assert np.array_equal(out, flags)
    assert (e_t[0, 0, :, 20][~np.isnan(e_t[0, 0, :, 20])] == 0).all() and (e_f[1, 0, 5][~np.isnan(e_f[1, 0, 5])] == 0).all()
    assert np.isnan(e_t[:, :, :, 7]).all() and np.isnan(e_f[:, :, 11]).all()
    ends = chunk_ends(50, 120)
    assert (np.diff(ends) == 0).any() and (np.diff(ends) == 1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("windows", [(3, 3), (5, 9)], ids=["w3", "w5-9"])
def test_gpu_nonfinite_samples(gpu, windows, dtype):
    """Unflagged NaN samples and unflagged (inf, x), (x, inf), (inf, NaN) samples, and a flagged infinite one."""
    vis, flags = make_case((2, 2, 30, 44), 80, 0.05, dtype, special=True)
    kw = dict(DEFAULTS, window_time=windows[0], window_freq=windows[1], scale_time=1.8, scale_freq=1.8, freq_chunks=3)
    with compared():
        e_t, e_f, out = check(("nonfinite", windows, dtype), vis, flags, kw)
        check(("nonfinite", windows, dtype), vis, flags, kw, offset=True)
    assert np.isposinf(e_t).any() and np.isposinf(e_f).any() and np.isnan(e_t[~flags]).any()
    assert out[np.isposinf(e_t) | np.isposinf(e_f)].all()


@pytest.mark.gpu
def test_gpu_batching_gives_the_same_result(gpu):
    vis, flags = make_case((3, 2, 21, 36), 90, 0.05)
    kw = dict(DEFAULTS, scale_time=1.8, scale_freq=1.8, freq_chunks=3)
    with compared():
        check("batch", vis, flags, kw)
        check("batch", vis, flags, kw, max_windows=1)
        check("batch", vis, flags, kw, max_windows=4)


@pytest.mark.gpu
def test_gpu_noise_and_scrambled_patch(gpu):
    """The two behaviour inputs of the CPU tests with the default kwargs, on the device."""
    vis, flags = noise_input(seed=1)
    with compared():
        _, _, out = check("noise", vis[None, None], flags[None, None], dict(DEFAULTS))
    assert np.array_equal(out[0, 0], flags)
    vis, flags, patch = scrambled_patch_input()
    with compared():
        _, _, out = check("patch", vis[None, None], flags[None, None], dict(DEFAULTS))
    assert (out[0, 0] & ~flags)[patch].all()


@pytest.mark.gpu
def test_gpu_apply_strategies_with_the_step_in_a_chain(gpu):
    import torch
    from tricolour_amd import flagging
    from tricolour_amd.strategies import apply_strategies
    vis, flags = make_case((3, 2, 40, 64), 100, 0.03)
    vis[..., 20:22] *= np.float32(8)
    st_kw = dict(num_major_iterations=1, background_iterations=1)
    kw = dict(DEFAULTS, scale_time=2.0, scale_freq=2.0, freq_chunks=2)
    v, f = dev(torch, vis), dev(torch, flags)
    with compared():
        got = apply_strategies([{"task": "sum_threshold", "kwargs": st_kw}, {"task": TASK, "kwargs": kw},
                                {"task": "combine_with_input_flags"}], f, v)
        st = (flagging.sum_threshold_flagger(v, f, **st_kw) | f).cpu().numpy()
        exp = restate_threshold(vis, st, **kw) | st | flags
        assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), exp)
    assert (exp & ~st).any() and not exp.all()


@pytest.mark.gpu
def test_gpu_flag_scan_whole_and_chunked(gpu):
    from tricolour_amd import scan
    from test_baseline_integrated import small_scan
    from test_scan_gpu import _plain
    data, flag, ant1, ant2, tm, freq, width = small_scan(np.random.RandomState(41))
    data[::7, 30:33, :] *= np.exp(2j * np.pi * np.random.RandomState(42).uniform(size=(data[::7].shape[0], 3, 1))).astype(np.complex64) * 6
    strategies = [{"task": "flag_autos"}, {"task": TASK, "kwargs": dict(DEFAULTS, scale_time=2.0, scale_freq=2.0, freq_chunks=2)}]
    with compared():
        whole, w_orig, w_final = scan.flag_scan(data, flag, ant1, ant2, tm, freq, width, strategies)
        chunked, c_orig, c_final = scan.flag_scan(data, flag, ant1, ant2, tm, freq, width, strategies, baseline_chunks=2)
        assert isinstance(whole, np.ndarray) and np.array_equal(whole, chunked)
        assert _plain(w_orig) == _plain(c_orig) and _plain(w_final) == _plain(c_final)
        base, _, _ = scan.flag_scan(data, flag, ant1, ant2, tm, freq, width, strategies[:1])
        assert (whole >= base).all() and (whole != base).any() and not whole.all()
        ds = dict(DATA=data, FLAG=flag, ANTENNA1=ant1, ANTENNA2=ant2, TIME=tm, CHAN_FREQ=freq, CHAN_WIDTH=width,
                  FIELD_ID=0, DATA_DESC_ID=0, SCAN_NUMBER=1)
        a, sa = scan.flag_scans([ds], strategies)
        b, sb = scan.flag_scans([ds], strategies, baseline_chunks=2)
        assert sa == sb and np.array_equal(np.asarray(a[0]), np.asarray(b[0])) and np.array_equal(np.asarray(a[0]), whole)


@pytest.mark.gpu
def test_gpu_every_listed_kernel_instantiation_was_launched_and_compared(gpu):
    """One compared call per route (the tests above add theirs when they ran): each launches exactly the instantiations
    its dtype, windows and alignment select, and together they are the table."""
    vi = {"c64": 0, "f32": 1}
    for dtype in ("c64", "f32"):
        for wt, wf in ((3, 5), (5, 9), (9, 3)):
            for offset in (False, True):
                shape = (2, 1, 10, 16)
                vis, flags = make_case(shape, 110 + wt, 0.05, dtype)
                kw = dict(DEFAULTS, window_time=wt, window_freq=wf, scale_time=1.8, scale_freq=1.8, freq_chunks=2)
                with compared() as log:
                    check(("routes", dtype, wt, wf), vis, flags, kw, offset=offset)
                vec = "false" if offset else "true"
                want = {"k_ldev_time<%d, %d, %s>" % (vi[dtype], wt if wt < 9 else 0, vec),
                        "k_ldev_freq<%d, %d, %s>" % (vi[dtype], wf if wf < 9 else 0, vec),
                        "k_ldev_level<0>", "k_ldev_level<1>", "k_ldev_apply<%s>" % vec}
                assert {k for k in log if k.startswith("k_ldev_")} == want, (dtype, wt, wf, offset, log)
    listed = set().union(*KERNELS.values())
    assert MET == listed, (sorted(listed - MET), sorted(MET - listed))
