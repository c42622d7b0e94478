"""Value-driven hysteresis growth of flags (``hysteresis_growth``): the NumPy
restatement of the five stages of the definition (``include/tricolour_amd.h``)
against a plain per-sample loop, its properties, its behaviour on skirts and on
noise and the strategy plumbing on the CPU; the device kernels against the
restatement on the GPU.

No tolerance anywhere.  The levels are exact selects and float32 operations in
a fixed order, the thresholds two correctly rounded float64 operations, the
growth integer logic: the four level arrays must agree in every bit, NaN
positions included, and both eligibility images and the flags must be equal.

This module also keeps the kernel table of ``tricolour_amd/csrc/steps/hyst/``:
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

TASK = "hysteresis_growth"
DEFAULTS = dict(nsigma_time=2.5, nsigma_freq=2.5, reach=8, freq_chunks=10)
NAN32 = np.uint32(0x7FC00000).view(np.float32)
MAD_NORMAL = 1.4826

# every __global__ kernel of csrc/steps/hyst/ and its instantiations, in the spelling of the kernel log
# (k_hyst_level<VIS, AXIS>, k_hyst_eligible<VIS>: VIS 0 = complex64, 1 = float32; k_hyst_grow<VEC>)
KERNELS = {
    "k_hyst_level": {"k_hyst_level<%d, %d>" % (v, a) for v in (0, 1) for a in (0, 1)},
    "k_hyst_eligible": {"k_hyst_eligible<0>", "k_hyst_eligible<1>"},
    "k_hyst_pack": {"k_hyst_pack"},
    "k_hyst_grow": {"k_hyst_grow<true>", "k_hyst_grow<false>"},
}
MET = set()        # instantiations launched by calls whose results equalled the restatement


# ---------------------------------------------------------------------------
# the definition, restated: plain loops over the lines for the levels, array rounds for the growth ...
# ---------------------------------------------------------------------------
def amplitude(vis):
    """Stage 1: float32, +inf where a part is infinite."""
    vis = np.asarray(vis)
    if not np.iscomplexobj(vis):
        return np.abs(vis.astype(np.float32))
    re, im = vis.real.astype(np.float64), vis.imag.astype(np.float64)
    with np.errstate(all="ignore"):
        a = np.sqrt(re * re + im * im).astype(np.float32)
    a[np.isinf(vis.real) | np.isinf(vis.imag)] = np.inf
    return a


def median32(values):
    """The library's median of a float32 vector (not empty)."""
    s = np.sort(np.asarray(values, np.float32))
    m = len(s)
    if m % 2:
        return s[(m - 1) // 2]
    with np.errstate(over="ignore"):
        return np.float32(np.float32(s[m // 2 - 1] + s[m // 2]) / np.float32(2))


def line_levels(a, counts):
    """Stage 2 for one line: (med, mad), both NaN when the line is not live."""
    vals = a[counts & np.isfinite(a)]
    if len(vals) >= 3:
        med = median32(vals)
        if np.isfinite(med):
            mad = median32(np.abs((vals - med).astype(np.float32)))
            if np.isfinite(mad) and mad > 0:
                return med, mad
    return NAN32, NAN32


def chunk_ends(nchan, freq_chunks):
    return np.linspace(0, nchan, freq_chunks + 1).astype(int)


def restate_levels(vis, flags, freq_chunks=10):
    """(med_t, mad_t, med_f, mad_f) of (..., time, chan) inputs."""
    a = amplitude(vis)
    counts = (np.asarray(flags) == 0) & ~np.isnan(a)
    lead, (T, F) = a.shape[:-2], a.shape[-2:]
    ends = chunk_ends(F, freq_chunks)
    med_t, mad_t = np.full(lead + (F,), NAN32), np.full(lead + (F,), NAN32)
    med_f, mad_f = np.full(lead + (T, freq_chunks), NAN32), np.full(lead + (T, freq_chunks), NAN32)
    for w in np.ndindex(*lead):
        for c in range(F):
            med_t[w + (c,)], mad_t[w + (c,)] = line_levels(a[w][:, c], counts[w][:, c])
        for t in range(T):
            for k in range(freq_chunks):
                lo, hi = ends[k], ends[k + 1]
                if hi > lo:
                    med_f[w + (t, k)], mad_f[w + (t, k)] = line_levels(a[w][t, lo:hi], counts[w][t, lo:hi])
    return med_t, mad_t, med_f, mad_f


def _eligible(a, counts, med, mad, nsigma):
    if nsigma == 0:
        return np.zeros(a.shape, bool)
    with np.errstate(invalid="ignore"):
        spread = (np.float64(nsigma) * MAD_NORMAL) * mad.astype(np.float64)       # rounded before the sum
        thr = med.astype(np.float64) + spread
        over = ~np.isnan(med) & (a.astype(np.float64) > thr)
    return counts & (np.isposinf(a) | over)


def restate_eligibility(vis, flags, nsigma_time=2.5, nsigma_freq=2.5, freq_chunks=10, levels=None):
    """Stage 3: (e_time, e_freq)."""
    a = amplitude(vis)
    counts = (np.asarray(flags) == 0) & ~np.isnan(a)
    med_t, mad_t, med_f, mad_f = levels if levels is not None else restate_levels(vis, flags, freq_chunks)
    ends = chunk_ends(a.shape[-1], freq_chunks)
    which = np.searchsorted(ends, np.arange(a.shape[-1]), side="right") - 1       # the chunk of every channel
    e_t = _eligible(a, counts, med_t[..., None, :], mad_t[..., None, :], nsigma_time)
    e_f = _eligible(a, counts, med_f[..., which], mad_f[..., which], nsigma_freq) if a.shape[-1] else np.zeros(a.shape, bool)
    return e_t, e_f


def restate_grow(seeds, e_time, e_freq, reach):
    """Stage 5: G_reach; every round reads the previous one, nothing beyond the edges."""
    g = np.asarray(seeds) != 0
    e_time, e_freq = np.asarray(e_time) != 0, np.asarray(e_freq) != 0
    for _ in range(reach):
        tn, fn = np.zeros_like(g), np.zeros_like(g)
        tn[..., 1:, :] |= g[..., :-1, :]
        tn[..., :-1, :] |= g[..., 1:, :]
        fn[..., 1:] |= g[..., :-1]
        fn[..., :-1] |= g[..., 1:]
        g = g | (e_time & tn) | (e_freq & fn)
    return g


def restate(vis, flags, missing=None, nsigma_time=2.5, nsigma_freq=2.5, reach=8, freq_chunks=10, parts=None):
    """out of the whole step (stage 4: the seeds)."""
    f = np.asarray(flags) != 0
    e_t, e_f = parts if parts is not None else restate_eligibility(vis, flags, nsigma_time, nsigma_freq, freq_chunks)
    seeds = f if missing is None else f & ~(np.asarray(missing) != 0)
    return f | restate_grow(seeds, e_t, e_f, reach)


# ---------------------------------------------------------------------------
# ... and as a plain per-sample loop over one (time, chan) window
# ---------------------------------------------------------------------------
def loop_step(vis, flags, missing, nsigma_time, nsigma_freq, reach, freq_chunks):
    T, F = vis.shape
    a = [[None] * F for _ in range(T)]
    for t in range(T):
        for c in range(F):
            z = vis[t, c]
            if np.iscomplexobj(vis):
                re, im = np.float32(z.real), np.float32(z.imag)
                if math.isinf(re) or math.isinf(im):
                    a[t][c] = np.float32(np.inf)
                else:
                    with np.errstate(over="ignore"):
                        a[t][c] = np.float32(math.sqrt(float(re) * float(re) + float(im) * float(im)))
            else:
                a[t][c] = np.float32(abs(np.float32(z)))
    counts = [[(not flags[t, c]) and not math.isnan(a[t][c]) for c in range(F)] for t in range(T)]

    def median(vals):
        vals = sorted(vals)
        m = len(vals)
        if m % 2:
            return vals[(m - 1) // 2]
        with np.errstate(over="ignore"):
            return np.float32(np.float32(vals[m // 2 - 1] + vals[m // 2]) / np.float32(2))

    def levels(cells):
        vals = [a[t][c] for t, c in cells if counts[t][c] and math.isfinite(a[t][c])]
        if len(vals) < 3:
            return None
        med = median(vals)
        if not math.isfinite(med):
            return None
        mad = median([np.float32(abs(np.float32(v - med))) for v in vals])
        if not math.isfinite(mad) or not mad > 0:
            return None
        return med, mad

    def eligible(t, c, lev, nsigma):
        if nsigma == 0 or not counts[t][c]:
            return False
        if a[t][c] == np.inf:
            return True
        if lev is None:
            return False
        spread = (float(nsigma) * MAD_NORMAL) * float(lev[1])
        return float(a[t][c]) > float(lev[0]) + spread

    ends = chunk_ends(F, freq_chunks)
    lev_t = [levels([(t, c) for t in range(T)]) for c in range(F)]
    e_t = [[eligible(t, c, lev_t[c], nsigma_time) for c in range(F)] for t in range(T)]
    e_f = [[False] * F for _ in range(T)]
    for t in range(T):
        for lo, hi in zip(ends[:-1], ends[1:]):
            lev = levels([(t, c) for c in range(lo, hi)])
            for c in range(lo, hi):
                e_f[t][c] = eligible(t, c, lev, nsigma_freq)
    g = [[bool(flags[t, c]) and not (missing is not None and missing[t, c]) for c in range(F)] for t in range(T)]
    for _ in range(reach):
        new = [row[:] for row in g]
        for t in range(T):
            for c in range(F):
                tn = (t > 0 and g[t - 1][c]) or (t + 1 < T and g[t + 1][c])
                fn = (c > 0 and g[t][c - 1]) or (c + 1 < F and g[t][c + 1])
                new[t][c] = g[t][c] or (e_t[t][c] and tn) or (e_f[t][c] and fn)
        g = new
    out = np.array([[bool(flags[t, c]) or g[t][c] for c in range(F)] for t in range(T)])
    return np.array(e_t, bool), np.array(e_f, bool), out


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
    """Noise whose level varies over 6 decades from channel to channel, a fifth of the samples raised by 2 to 6 (the
    eligible ones: long winding paths), `density` input flags; special: unflagged NaN and infinite samples, a flagged
    infinite one, a channel and a row flagged throughout, a line of identical values (mad 0)."""
    rng = np.random.default_rng(seed)
    if dtype == "c64":
        vis = np.empty(shape, np.complex64)
        vis.real = rng.standard_normal(shape, dtype=np.float32)
        vis.imag = rng.standard_normal(shape, dtype=np.float32)
    else:
        vis = rng.standard_normal(shape, dtype=np.float32)
    vis *= (10.0 ** rng.uniform(-3.0, 3.0, size=(shape[0], 1, 1, shape[3]))).astype(np.float32)
    high = rng.uniform(size=shape) < 0.2
    vis[high] *= rng.uniform(2.0, 6.0, size=int(high.sum())).astype(np.float32)
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
        if flat.size > 8:
            q = int(pos[0] + 1) % flat.size
            if q not in pos:
                flat[q] = np.inf
                fl[q] = True
        if shape[2] > 12 and shape[3] > 21:
            flags[:, :, :, 7] = True
            flags[:, :, 11, :] = True
            vis[0, 0, :, 20] = vis[0, 0, 0, 20]
            vis[-1, 0, 5, :] = vis[-1, 0, 5, 0]
    return vis, flags


_CACHE = {}


def expected(key, vis, flags, kw, missing=None):
    """(levels, (e_time, e_freq), out) of the restatement; computed once per key and left unchanged."""
    if key not in _CACHE:
        levels = restate_levels(vis, flags, kw["freq_chunks"])
        parts = restate_eligibility(vis, flags, kw["nsigma_time"], kw["nsigma_freq"], kw["freq_chunks"], levels=levels)
        _CACHE[key] = (levels, parts, restate(vis, flags, missing, parts=parts, reach=kw["reach"]))
    return _CACHE[key]


def phases(rs, n):
    return np.exp(2j * np.pi * rs.rand(n))


def skirt_input(s):
    """Unit complex noise on 96 x 160; row 40 and channel 100 carry an added amplitude of 12 and are flagged (the seeds),
    rows 39 and 41 and channels 99 and 101 an added amplitude of 5, unflagged (the skirts); a fresh uniform phase per cell,
    the larger amplitude where regions overlap."""
    rs = np.random.RandomState(100 + s)
    shape = (96, 160)
    vis = rs.randn(*shape) + 1j * rs.randn(*shape)
    amp = np.zeros(shape)
    skirt_rows, skirt_cols = np.zeros(shape, bool), np.zeros(shape, bool)
    skirt_rows[[39, 41], :] = True
    skirt_cols[:, [99, 101]] = True
    amp[skirt_rows | skirt_cols] = 5.0
    seeds = np.zeros(shape, bool)
    seeds[40, :] = True
    seeds[:, 100] = True
    amp[seeds] = 12.0
    vis = (vis + amp * phases(rs, vis.size).reshape(shape)).astype(np.complex64)
    return vis, seeds, skirt_rows & ~seeds, skirt_cols & ~seeds


SKIRT_KW = dict(nsigma_time=2.5, nsigma_freq=2.5, reach=8, freq_chunks=2)


def assert_skirts(new, seeds, skirt_rows, skirt_cols):
    assert not (new & seeds).any()
    assert new[skirt_rows].mean() >= 0.90 and new[skirt_cols].mean() >= 0.90, (new[skirt_rows].mean(), new[skirt_cols].mean())
    other = new & ~(skirt_rows | skirt_cols)
    assert other.sum() <= 20, int(other.sum())
    near = np.zeros(new.shape, bool)
    near[37:44, :] = True
    near[:, 97:104] = True
    assert not (new & ~near).any(), int((new & ~near).sum())


def noise_input(s):
    rs = np.random.RandomState(100 + s)
    shape = (96, 160)
    vis = (rs.randn(*shape) + 1j * rs.randn(*shape)).astype(np.complex64)
    return vis, rs.rand(*shape) < 0.02


def path_distance(flags, limit):
    """City-block distance to the nearest flag, up to limit + 1."""
    d = np.where(flags, 0, limit + 1)
    for _ in range(limit):
        n = d.copy()
        n[1:] = np.minimum(n[1:], d[:-1] + 1)
        n[:-1] = np.minimum(n[:-1], d[1:] + 1)
        n[:, 1:] = np.minimum(n[:, 1:], d[:, :-1] + 1)
        n[:, :-1] = np.minimum(n[:, :-1], d[:, 1:] + 1)
        d = n
    return d


# ---------------------------------------------------------------------------
# CPU: the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["c64", "f32"])
def test_restatement_equals_the_per_sample_loop(dtype):
    cases = [(dict(DEFAULTS, freq_chunks=2), False, False), (dict(DEFAULTS, nsigma_time=1.0, nsigma_freq=0.5, reach=3, freq_chunks=3), True, True),
             (dict(DEFAULTS, nsigma_time=0.0, nsigma_freq=1.0, reach=32, freq_chunks=1), True, False),
             (dict(DEFAULTS, nsigma_time=1.0, nsigma_freq=0.0, reach=1, freq_chunks=20), False, True)]
    for i, (kw, special, masked) in enumerate(cases):
        vis, flags = make_case((1, 1, 7, 13), 10 + i, 0.1, dtype, special)
        vis[0, 0, :, 3] = vis[0, 0, 0, 3]                       # a line of identical values: mad 0
        missing = (np.random.default_rng(i).uniform(size=flags.shape) < 0.3) if masked else None
        e_t, e_f = restate_eligibility(vis, flags, kw["nsigma_time"], kw["nsigma_freq"], kw["freq_chunks"])
        out = restate(vis, flags, missing, **kw)
        l_t, l_f, l_out = loop_step(vis[0, 0], flags[0, 0], None if missing is None else missing[0, 0], **kw)
        assert np.array_equal(e_t[0, 0], l_t) and np.array_equal(e_f[0, 0], l_f), kw
        assert np.array_equal(out[0, 0], l_out), kw


def test_no_seeds_or_both_axes_off_add_nothing():
    vis, flags = make_case((2, 2, 20, 31), 20, 0.1, "c64", True)
    none = np.zeros(flags.shape, bool)
    assert np.array_equal(restate(vis, none, **DEFAULTS), none)
    assert np.array_equal(restate(vis, flags, missing=flags, **DEFAULTS), flags)       # every flag missing: no seed
    assert np.array_equal(restate(vis, flags, **dict(DEFAULTS, nsigma_time=0.0, nsigma_freq=0.0)), flags)
    out = restate(vis, flags, **dict(DEFAULTS, nsigma_time=1.0, nsigma_freq=1.0))
    assert (out >= flags).all() and (out & ~flags).any() and not out.all()
    # a stack of windows equals the windows one by one
    for b in range(2):
        for p in range(2):
            one = restate(vis[b:b + 1, p:p + 1], flags[b:b + 1, p:p + 1], **dict(DEFAULTS, nsigma_time=1.0, nsigma_freq=1.0))
            assert np.array_equal(out[b, p], one[0, 0])


def test_a_flagged_sample_that_is_no_seed_blocks_growth():
    """14 strong samples in a row, one of them the seed: growth runs along them until a flagged, missing sample, and
    not beyond."""
    rs = np.random.RandomState(5)
    vis = (rs.randn(1, 1, 21, 40) + 1j * rs.randn(1, 1, 21, 40)).astype(np.complex64)
    vis[0, 0, 10, :14] += 30
    flags = np.zeros(vis.shape, bool)
    flags[0, 0, 10, 5] = True                       # the seed
    flags[0, 0, 10, 9] = True                       # flagged, missing
    missing = np.zeros(vis.shape, bool)
    missing[0, 0, 10, 9] = True
    kw = dict(DEFAULTS, nsigma_time=0.0, nsigma_freq=6.0, reach=32, freq_chunks=1)
    e_t, e_f = restate_eligibility(vis, flags, kw["nsigma_time"], kw["nsigma_freq"], kw["freq_chunks"])
    assert not e_t.any() and not e_f[flags].any() and e_f.sum() == 12 and e_f[0, 0, 10, :14].sum() == 12
    out = restate(vis, flags, missing, **kw)
    assert out[0, 0, 10, :10].all() and out.sum() == 10
    out = restate(vis, flags, None, **kw)           # as a seed it grows on
    assert out[0, 0, 10, :14].all() and out.sum() == 14


def test_nonfinite_samples():
    rs = np.random.RandomState(6)
    vis = (rs.randn(1, 1, 9, 30) + 1j * rs.randn(1, 1, 9, 30)).astype(np.complex64)
    flags = np.zeros(vis.shape, bool)
    flags[0, 0, 4, 10] = True
    vis[0, 0, 4, 11] = complex(np.inf, 1.0)         # eligible next to the seed
    vis[0, 0, 4, 9] = complex(np.nan, 1.0)          # never eligible
    vis[0, 0, 3, 10] = complex(np.inf, np.nan)      # a part is infinite: a = +inf, it counts
    vis[0, 0, 7, 20] = np.inf                        # far from any seed
    kw = dict(DEFAULTS, nsigma_time=1e6, nsigma_freq=1e6, freq_chunks=1)
    e_t, e_f = restate_eligibility(vis, flags, kw["nsigma_time"], kw["nsigma_freq"], kw["freq_chunks"])
    assert e_t.sum() == 3 and e_f.sum() == 3 and not e_t[0, 0, 4, 9] and not e_f[0, 0, 4, 9]
    exp = flags.copy()
    exp[0, 0, 4, 11] = True
    exp[0, 0, 3, 10] = True
    assert np.array_equal(restate(vis, flags, **kw), exp)
    finite = vis.copy()
    finite[0, 0, 4, 11] = finite[0, 0, 4, 9] = finite[0, 0, 3, 10] = finite[0, 0, 7, 20] = 1.0
    held = flags.copy()
    held[0, 0, 4, 11] = held[0, 0, 4, 9] = held[0, 0, 3, 10] = held[0, 0, 7, 20] = True
    for got, want in zip(restate_levels(vis, flags, 1), restate_levels(finite, held, 1)):
        assert same_bits(got, want)                 # neither enters a level


@pytest.mark.parametrize("s", range(6))
def test_behaviour_skirts_of_a_burst_and_a_carrier(s):
    vis, seeds, skirt_rows, skirt_cols = skirt_input(s)
    out = restate(vis[None, None], seeds[None, None], **SKIRT_KW)[0, 0]
    assert_skirts(out & ~seeds, seeds, skirt_rows, skirt_cols)


@pytest.mark.parametrize("s", range(3))
def test_behaviour_noise(s):
    vis, flags = noise_input(s)
    out = restate(vis[None, None], flags[None, None], **DEFAULTS)[0, 0]
    new = out & ~flags
    assert new.sum() <= 0.005 * flags.size, int(new.sum())
    assert not new[path_distance(flags, 8) > 8].any()


# ---------------------------------------------------------------------------
# CPU: plumbing
# ---------------------------------------------------------------------------
def test_the_task_is_valid_and_checked():
    from tricolour_amd import scan
    assert TASK in scan.VALID_TASKS and TASK not in scan.WHOLE_SCAN_TASKS
    scan.check_strategies([{"task": TASK}, {"task": TASK, "kwargs": dict(DEFAULTS)}, {"task": TASK, "kwargs": None},
                           {"task": TASK, "kwargs": dict(reach=1, nsigma_time=0, nsigma_freq=0.0, missing="none")},
                           {"task": TASK, "kwargs": dict(reach=32, freq_chunks=1, missing="input")},
                           {"task": "mark_missing"}, {"task": TASK, "kwargs": dict(missing="marked")}])
    bad = [dict(reach=0), dict(reach=33), dict(reach=2.5), dict(reach=True), dict(nsigma_time=-0.1), dict(nsigma_freq=-1),
           dict(nsigma_time=float("nan")), dict(nsigma_freq=float("nan")), dict(freq_chunks=0), dict(missing="other"),
           dict(missing="marked"), dict(window=3)]
    for kw in bad:
        with pytest.raises(ValueError, match=TASK):
            scan.check_strategies([{"task": "flag_autos"}, {"task": TASK, "kwargs": kw}])


def test_python_argument_errors_come_before_any_device_work():
    from tricolour_amd import flagging
    vis = np.zeros((3, 1, 4, 8), np.complex64)
    flags = np.zeros((3, 1, 4, 8), bool)
    for fn in (flagging.hysteresis_growth, flagging.robust_line_levels, flagging.growth_eligibility):
        with pytest.raises(ValueError):
            fn(vis, flags[:, :, :3])
        with pytest.raises(ValueError):
            fn(vis[0], flags[0])
        with pytest.raises(ValueError, match="freq_chunks"):
            fn(vis, flags, freq_chunks=0)
    for kw in (dict(reach=0), dict(reach=33), dict(reach=2.5), dict(reach=True), dict(nsigma_time=-1.0),
               dict(nsigma_freq=float("nan")), dict(missing=flags[:, :, :3])):
        with pytest.raises(ValueError):
            flagging.hysteresis_growth(vis, flags, **kw)
    for kw in (dict(nsigma_time=-1.0), dict(nsigma_freq=float("nan"))):
        with pytest.raises(ValueError, match="nsigma"):
            flagging.growth_eligibility(vis, flags, **kw)
    for args in ((flags, flags, flags, 0), (flags, flags, flags, 33), (flags, flags[:, :, :3], flags, 8),
                 (flags, flags, flags[..., :7], 8), (flags[0], flags[0], flags[0], 8)):
        with pytest.raises(ValueError):
            flagging.grow_flags(*args)
    with pytest.raises(ValueError, match="missing"):
        flagging.check_hysteresis_kwargs(missing="other")
    assert flagging.check_hysteresis_kwargs() == (2.5, 2.5, 8, 10, "none")


def test_header_declares_and_the_binding_exports_the_entry_points():
    from tricolour_amd import _lib
    with open(os.path.join(ROOT, "include", "tricolour_amd.h")) as fh:
        hdr = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name, res in (("tri_hyst_workspace_bytes", "size_t"), ("tri_hyst_levels", "int"), ("tri_hyst_eligible", "int"),
                      ("tri_hyst_grow", "int"), ("tri_hysteresis_growth", "int")):
        assert re.search(r"\b%s\s+%s\s*\(" % (res, name), hdr), name
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().tri_version() >= 106
    assert os.path.join(ROOT, "tricolour_amd", "csrc", "steps", "hyst", "kernels_hyst.hpp") in _lib.DEPENDS


def test_abi_rejects_bad_arguments_without_a_launch():
    import ctypes as C
    from tricolour_amd import _lib
    lib = _lib.lib()
    buf = (C.c_uint8 * 32768)()
    base = C.addressof(buf)
    v, f, o, a, b, c, d = (base + 4096 * i for i in range(7))
    ends = (C.c_int64 * 3)(0, 4, 8)

    def lev(vis=v, dtype=_lib.TRI_VIS_C64, flags=f, n_win=2, ntime=4, nchan=8, ce=ends, nce=3, m0=a, m1=b, m2=c, m3=d,
            ws=o, wsb=0):
        return lib.tri_hyst_levels(vis, dtype, flags, n_win, ntime, nchan, ce, nce, m0, m1, m2, m3, ws, wsb, None)

    def eli(vis=v, dtype=_lib.TRI_VIS_C64, flags=f, n_win=2, ntime=4, nchan=8, nt=2.5, nf=2.5, ce=ends, nce=3, et=a, ef=b,
            ws=o, wsb=0):
        return lib.tri_hyst_eligible(vis, dtype, flags, n_win, ntime, nchan, nt, nf, ce, nce, et, ef, ws, wsb, None)

    def grow(seeds=f, et=a, ef=b, out=c, n_win=2, ntime=4, nchan=8, reach=8, ws=o, wsb=0):
        return lib.tri_hyst_grow(seeds, et, ef, out, n_win, ntime, nchan, reach, ws, wsb, None)

    def step(vis=v, dtype=_lib.TRI_VIS_C64, flags=f, missing=None, out=c, n_win=2, ntime=4, nchan=8, nt=2.5, nf=2.5,
             reach=8, ce=ends, nce=3, ws=o, wsb=0):
        return lib.tri_hysteresis_growth(vis, dtype, flags, missing, out, n_win, ntime, nchan, nt, nf, reach, ce, nce,
                                         ws, wsb, None)
    for fn in (lev, eli, step):
        for kw in (dict(vis=None), dict(flags=None), dict(n_win=-1), dict(ntime=-1), dict(nchan=-1), dict(ce=None),
                   dict(nce=1), dict(nchan=9), dict(ce=(C.c_int64 * 3)(0, 5, 4)), dict(ce=(C.c_int64 * 3)(1, 4, 8))):
            assert fn(**kw) == _lib.TRI_EINVAL, (fn.__name__, kw)
        for dt in (_lib.TRI_VIS_C128, _lib.TRI_VIS_F64, 17, -1):
            assert fn(dtype=dt) == _lib.TRI_EUNSUPPORTED
        assert fn(n_win=0) == _lib.TRI_OK and fn(ntime=0) == _lib.TRI_OK               # empty: no launch
        assert fn(nchan=0, ce=(C.c_int64 * 2)(0, 0), nce=2) == _lib.TRI_OK
        assert fn() == _lib.TRI_EWORKSPACE and fn(ws=None, wsb=1 << 30) == _lib.TRI_EWORKSPACE
    for fn in (eli, step):
        for kw in (dict(nt=-1.0), dict(nf=float("nan"))):
            assert fn(**kw) == _lib.TRI_EINVAL, (fn.__name__, kw)
    for fn in (grow, step):
        for kw in (dict(reach=0), dict(reach=33), dict(reach=-1), dict(out=None), dict(out=f + 8)):
            assert fn(**kw) == _lib.TRI_EINVAL, (fn.__name__, kw)
    for kw in (dict(m0=None), dict(m3=None)):
        assert lev(**kw) == _lib.TRI_EINVAL
    for kw in (dict(et=None), dict(ef=None), dict(et=f + 8), dict(ef=a + 8)):
        assert eli(**kw) == _lib.TRI_EINVAL
    for kw in (dict(seeds=None), dict(et=None), dict(ef=None), dict(n_win=-1), dict(out=a + 8), dict(out=b)):
        assert grow(**kw) == _lib.TRI_EINVAL
    assert step(missing=c + 8) == _lib.TRI_EINVAL
    assert grow(n_win=0) == _lib.TRI_OK and grow(nchan=0) == _lib.TRI_OK
    assert grow() == _lib.TRI_EWORKSPACE and grow(ws=None, wsb=1 << 30) == _lib.TRI_EWORKSPACE
    need = lib.tri_hyst_workspace_bytes(2, 4, 8, 3)
    assert need >= 3 * 2 * 4 * 4 + 2 * 2 * 8 * 4 + 2 * 2 * 4 * 2 * 4 + 24 and step(wsb=need - 1) == _lib.TRI_EWORKSPACE
    assert lib.tri_hyst_workspace_bytes(0, 4, 8, 3) == 0 and lib.tri_hyst_workspace_bytes(2, 4, 8, 1) == 0
    assert lib.tri_hyst_workspace_bytes(64, 4, 8, 3) > need
    # 3 bits per sample and the levels: 0.40 byte per sample at the benchmark's window shape
    assert lib.tri_hyst_workspace_bytes(4, 1024, 4096, 11) < 0.41 * 4 * 1024 * 4096


# ---------------------------------------------------------------------------
# CPU: the kernel table against the sources
# ---------------------------------------------------------------------------
def scan_hyst_kernels():
    found = set()
    paths = sorted(glob.glob(os.path.join(ROOT, "tricolour_amd", "csrc", "steps", "hyst", "*")))
    assert paths
    for path in paths:
        with open(path, encoding="utf-8") as fh:
            found.update(re.findall(r"__global__[\s\S]{0,200}?\b(k_\w+)\s*\(", fh.read()))
    return found


def test_kernel_table_lists_what_the_sources_hold():
    from test_route_ledger import scan_instances, scan_kernels
    assert scan_hyst_kernels() == set(KERNELS)
    assert not set(KERNELS) & scan_kernels()                   # the ledger keeps the kernels directly under csrc/
    sites = scan_instances()                                   # launch sites of the host code, macros expanded
    for kernel, instances in KERNELS.items():
        assert sites.get(kernel) == instances, kernel
    with open(os.path.join(ROOT, "tricolour_amd", "csrc", "tricolour_amd.hip"), encoding="utf-8") as fh:
        assert '#include "steps/hyst/kernels_hyst.hpp"' in fh.read()


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
    MET.update(k for k in log if k.startswith("k_hyst_"))


def dev(torch, a, offset=False):
    """A device copy of `a`; offset: a contiguous view whose base lies one element past an aligned address."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        return t.cuda()
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    flat[1:] = t.reshape(-1).cuda()
    return flat[1:].view(t.shape)


def differing(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


def check(key, vis, flags, kw, missing=None, container="tensor", offset=False, max_windows=None):
    """robust_line_levels, growth_eligibility, grow_flags and hysteresis_growth on the device against the restatement:
    the bits of the four level arrays, both eligibility images, the grown seeds, the flags, the results' container and
    dtype, and the inputs unchanged."""
    import torch
    from tricolour_amd import flagging
    e_lev, (e_t, e_f), e_out = expected(key, vis, flags, kw, missing)
    extra = {} if max_windows is None else dict(_max_windows=max_windows)
    if container == "numpy":
        v, f, m = vis.copy(), flags.copy(), None if missing is None else missing.copy()
    else:
        v, f = dev(torch, vis, offset), dev(torch, flags, offset)
        m = None if missing is None else dev(torch, missing, offset)
        if offset and vis.size:
            assert v.data_ptr() % 16 != 0
        f0 = f.clone()
    lev = flagging.robust_line_levels(v, f, freq_chunks=kw["freq_chunks"], **extra)
    g_t, g_f = flagging.growth_eligibility(v, f, kw["nsigma_time"], kw["nsigma_freq"], kw["freq_chunks"], **extra)
    grown = flagging.grow_flags(f, g_t, g_f, kw["reach"], **extra)
    out = flagging.hysteresis_growth(v, f, missing=m, **kw, **extra)
    if container == "numpy":
        assert all(isinstance(x, np.ndarray) for x in lev + (g_t, g_f, grown, out))
        assert out.dtype == flags.dtype and grown.dtype == flags.dtype and g_t.dtype == np.bool_ and g_f.dtype == np.bool_
        assert same_bits(v, vis) and np.array_equal(f, flags) and (m is None or np.array_equal(m, missing))
    else:
        assert all(x.is_cuda for x in lev + (g_t, g_f, grown, out))
        assert out.dtype == f.dtype and grown.dtype == f.dtype and g_t.dtype == torch.bool and g_f.dtype == torch.bool
        assert same_bits(v.cpu().numpy(), vis) and torch.equal(f, f0)
        lev = tuple(x.cpu().numpy() for x in lev)
        g_t, g_f, grown, out = (x.cpu().numpy() for x in (g_t, g_f, grown, out))
    for name, got, want in zip(("med_t", "mad_t", "med_f", "mad_f"), lev, e_lev):
        assert got.dtype == np.float32 and got.shape == want.shape, (key, name, got.shape, want.shape)
        assert differing(got, want) == 0, "%s: %d %s bit patterns differ" % (key, differing(got, want), name)
    bad_t, bad_f = int((g_t != e_t).sum()), int((g_f != e_f).sum())
    assert g_t.shape == e_t.shape and bad_t == 0 and bad_f == 0, "%s: %d e_time and %d e_freq differ" % (key, bad_t, bad_f)
    e_grown = restate_grow(flags, e_t, e_f, kw["reach"])
    nbad = int(((grown != 0) != e_grown).sum())
    assert nbad == 0, "%s: %d grown seeds differ" % (key, nbad)
    nbad = int(((out != 0) != e_out).sum())
    assert out.shape == e_out.shape and nbad == 0, "%s: %d flags differ" % (key, nbad)
    return e_lev, (e_t, e_f), e_out


KW = dict(nsigma_time=1.0, nsigma_freq=1.0, reach=8, freq_chunks=3)     # low thresholds: a fifth of the samples are eligible

SHAPES = [
    ((1, 1, 1, 40), {}), ((2, 1, 40, 1), {}), ((1, 1, 2, 3), {}),
    ((3, 2, 67, 133), {}), ((3, 2, 67, 133), dict(reach=1)), ((3, 2, 67, 133), dict(reach=2, freq_chunks=1)),
    ((3, 2, 67, 133), dict(reach=31, freq_chunks=10)), ((3, 2, 67, 133), dict(reach=32, freq_chunks=200)),
    # ntime one row beyond the growth tile (64 rows) and beyond the level strip (1024 rows), around the words' ends
    ((1, 1, 65, 31), {}), ((1, 1, 65, 32), {}), ((1, 1, 65, 33), {}), ((1, 1, 65, 63), {}), ((1, 1, 65, 64), {}),
    ((1, 1, 65, 65), {}), ((1, 1, 1025, 31), dict(reach=32)), ((1, 1, 1025, 32), {}), ((1, 1, 1025, 33), {}),
    ((1, 1, 1025, 63), {}), ((1, 1, 1025, 64), dict(reach=31)), ((1, 1, 1025, 65), dict(reach=2)),
    # one word and one row beyond every tile: 64 rows x 16 words (growth), 8 rows x 256 channels (eligibility), 1024 rows
    # and a chunk of 1024 channels (the levels' LDS strips), 8 channels and 4 lines per block (levels)
    ((1, 2, 1025, 1057), dict(freq_chunks=1)), ((1, 1, 130, 1072), dict(reach=32, freq_chunks=1)),
]


def shape_id(p):
    return "x".join(map(str, p[0])) + "".join("-%s%s" % (k[0], v) for k, v in sorted(p[1].items()))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("case", SHAPES, ids=shape_id)
def test_gpu_shapes_reaches_and_chunks(gpu, case, dtype):
    """Aligned (16 flags per lane where nchan % 16 == 0) and at a one-element offset (the bytewise route), as tensors."""
    shape, over = case
    kw = dict(KW, **over)
    vis, flags = make_case(shape, 40 + sum(shape), 0.01, dtype, special=True)
    key = ("shape", shape_id(case), dtype)
    with compared():
        _, _, out = check(key, vis, flags, kw)
        check(key, vis, flags, kw, offset=True)
    if min(shape[2:]) >= 31:
        assert (out & ~flags).any() and not out.all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("container", ["numpy", "tensor"])
def test_gpu_containers(gpu, container, dtype):
    import torch
    from tricolour_amd import flagging
    vis, flags = make_case((2, 2, 33, 52), 60, 0.03, dtype, special=True)
    missing = np.random.default_rng(61).uniform(size=flags.shape) < 0.5
    with compared():
        _, _, e_out = check(("containers", dtype), vis, flags, KW, missing=missing, container=container)
        if container == "tensor":                              # uint8 flags with any nonzero byte: uint8 0 / 1 comes back
            f3 = dev(torch, flags.astype(np.uint8) * 3)
            out = flagging.hysteresis_growth(dev(torch, vis), f3, missing=dev(torch, missing.astype(np.uint8) * 7), **KW)
            assert out.is_cuda and out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), e_out.astype(np.uint8))
            assert torch.equal(f3, dev(torch, flags.astype(np.uint8) * 3))
        else:
            out = flagging.hysteresis_growth(vis, flags.astype(np.uint8) * 5, missing=missing, **KW)
            assert out.dtype == np.uint8 and np.array_equal(out, e_out.astype(np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
def test_gpu_axes_chunks_and_missing(gpu, dtype):
    """freq_chunks 1, 3, 10 and more than F (empty chunks, chunks of one and two channels), each axis alone and both
    off, with and without a missing mask."""
    shape = (2, 1, 37, 50)
    vis, flags = make_case(shape, 70, 0.03, dtype, special=True)
    missing = np.random.default_rng(71).uniform(size=shape) < 0.5
    for chunks in (1, 3, 10, 120):
        for nt, nf in ((1.0, 1.0), (1.0, 0.0), (0.0, 1.0), (0.0, 0.0)):
            for m in (None, missing):
                kw = dict(KW, nsigma_time=nt, nsigma_freq=nf, freq_chunks=chunks)
                with compared():
                    _, _, out = check(("axes", dtype, chunks, nt, nf, m is None), vis, flags, kw, missing=m)
                if nt == 0.0 and nf == 0.0:
                    assert np.array_equal(out, flags)
    ends = chunk_ends(50, 120)
    assert (np.diff(ends) == 0).any() and (np.diff(ends) == 1).any()


GROW_SHAPES = [(1, 1, 1, 40), (2, 1, 40, 1), (1, 1, 2, 3), (3, 2, 67, 133), (1, 1, 65, 31), (1, 1, 65, 32), (1, 1, 65, 33),
               (1, 1, 65, 63), (1, 1, 65, 64), (1, 1, 65, 65), (2, 1, 130, 1072)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", GROW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gpu_grow_flags_on_random_planes(gpu, shape):
    """Seeds 1 %, eligibility 60 %: long, winding paths; every reach; aligned and at a one-byte offset."""
    import torch
    from tricolour_amd import flagging
    rng = np.random.default_rng(sum(shape))
    seeds, e_t, e_f = rng.uniform(size=shape) < 0.01, rng.uniform(size=shape) < 0.6, rng.uniform(size=shape) < 0.6
    for reach in (1, 2, 8, 31, 32):
        want = restate_grow(seeds, e_t, e_f, reach)
        for offset in (False, True):
            with compared():
                got = flagging.grow_flags(dev(torch, seeds, offset), dev(torch, e_t, offset), dev(torch, e_f, offset), reach)
                assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want), (shape, reach, offset)
    if seeds.any() and min(shape[2:]) > 40:
        assert (want & ~seeds).any() and not want.all()
        assert (want != restate_grow(seeds, e_t, e_f, 2)).any()           # paths longer than 2 steps exist


@pytest.mark.gpu
def test_gpu_grow_flags_lines_corners_and_window_edges(gpu):
    import torch
    from tricolour_amd import flagging
    T, F = 150, 140
    none = np.zeros((1, 1, T, F), bool)
    for reach in (1, 2, 8, 31, 32):
        # a line of 70 eligible cells from one seed along each axis, across channels 31 / 32 and 63 / 64 and rows 63 / 64
        for c0 in (20, 40):
            seeds, e = none.copy(), none.copy()
            seeds[0, 0, 5, c0] = True
            e[0, 0, 5, c0 + 1:c0 + 71] = True
            seeds[0, 0, 80, c0 + 80] = True
            e[0, 0, 80, c0 + 9:c0 + 80] = True                 # ... and downwards in channel
            want = seeds.copy()
            want[0, 0, 5, c0:c0 + reach + 1] = True
            want[0, 0, 80, c0 + 80 - reach:c0 + 81] = True
            with compared():
                got = flagging.grow_flags(dev(torch, seeds), dev(torch, none), dev(torch, e), reach).cpu().numpy()
                assert np.array_equal(got, want), (reach, c0)
                got = flagging.grow_flags(dev(torch, seeds), dev(torch, e), dev(torch, none), reach).cpu().numpy()
                assert np.array_equal(got, seeds), (reach, c0)                     # eligible on the other axis only
        for t0 in (30, 50):
            seeds, e = none.copy(), none.copy()
            seeds[0, 0, t0, 7] = True
            e[0, 0, t0 + 1:t0 + 71, 7] = True
            seeds[0, 0, t0 + 90, 100] = True
            e[0, 0, t0 + 19:t0 + 90, 100] = True
            want = seeds.copy()
            want[0, 0, t0:t0 + reach + 1, 7] = True
            want[0, 0, t0 + 90 - reach:t0 + 91, 100] = True
            with compared():
                got = flagging.grow_flags(dev(torch, seeds), dev(torch, e), dev(torch, none), reach).cpu().numpy()
                assert np.array_equal(got, want), (reach, t0)
        # a seed in every corner, everything eligible: four triangles
        seeds = none.copy()
        seeds[0, 0, [0, 0, -1, -1], [0, -1, 0, -1]] = True
        full = ~none
        t, c = np.meshgrid(np.arange(T), np.arange(F), indexing="ij")
        want = (np.minimum(t, T - 1 - t) + np.minimum(c, F - 1 - c) <= reach)[None, None]
        with compared():
            got = flagging.grow_flags(dev(torch, seeds), dev(torch, full), dev(torch, full), reach).cpu().numpy()
            assert np.array_equal(got, want), reach
    for F2 in (33, 64, 70):
        # two adjacent windows, one all seeds and one with none but all eligible: the second stays empty ...
        seeds = np.zeros((2, 1, 9, F2), bool)
        seeds[0] = True
        full = np.ones(seeds.shape, bool)
        with compared():
            got = flagging.grow_flags(dev(torch, seeds), dev(torch, full), dev(torch, full), 32).cpu().numpy()
            assert np.array_equal(got, seeds), F2
        # ... and nothing wraps from a row's last channel into the next row's first
        seeds = np.zeros((1, 1, 9, F2), bool)
        seeds[0, 0, 2, F2 - 1] = True
        e = np.zeros(seeds.shape, bool)
        e[0, 0, 3, :] = True
        e[0, 0, 1, :] = True
        with compared():
            got = flagging.grow_flags(dev(torch, seeds), dev(torch, np.zeros(seeds.shape, bool)), dev(torch, e), 8).cpu().numpy()
            assert np.array_equal(got, seeds), F2


@pytest.mark.gpu
def test_gpu_batching_gives_the_same_result(gpu):
    vis, flags = make_case((3, 2, 21, 36), 90, 0.03)
    with compared():
        check("batch", vis, flags, KW)
        check("batch", vis, flags, KW, max_windows=1)
        check("batch", vis, flags, KW, max_windows=4)


@pytest.mark.gpu
def test_gpu_behaviour_skirts(gpu):
    """The behaviour input of the CPU test on the device."""
    vis, seeds, skirt_rows, skirt_cols = skirt_input(0)
    with compared():
        _, _, out = check("skirts", vis[None, None], seeds[None, None], SKIRT_KW)
    assert_skirts(out[0, 0] & ~seeds, seeds, skirt_rows, skirt_cols)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["none", "input", "marked"])
def test_gpu_apply_strategies_with_the_step_in_a_chain(gpu, which):
    import torch
    from tricolour_amd import flagging
    from tricolour_amd.strategies import apply_strategies
    vis, flags = make_case((3, 2, 40, 64), 100, 0.03)
    vis[..., 20:22] *= np.float32(8)
    st_kw = dict(num_major_iterations=1, background_iterations=1)
    kw = dict(KW, freq_chunks=2)
    v, f = dev(torch, vis), dev(torch, flags)
    chain = [{"task": "sum_threshold", "kwargs": st_kw}, {"task": TASK, "kwargs": dict(kw, missing=which)}]
    if which == "marked":
        chain.insert(0, {"task": "mark_missing"})
    with compared():
        got = apply_strategies(chain, f, v)
        st = (flagging.sum_threshold_flagger(v, f, **st_kw) | f).cpu().numpy()
        exp = restate(vis, st, None if which == "none" else flags, **kw) | st
        assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), exp)
    assert (exp & ~st).any() and not exp.all()
    if which != "none":
        assert (exp != (restate(vis, st, None, **kw) | st)).any()                      # the mask matters here
    if which == "marked":
        with pytest.raises(ValueError, match=TASK):
            apply_strategies(chain[1:], f, v)


@pytest.mark.gpu
def test_gpu_flag_scan_whole_and_chunked(gpu):
    from tricolour_amd import scan
    from test_baseline_integrated import small_scan
    from test_scan_gpu import _plain
    data, flag, ant1, ant2, tm, freq, width = small_scan(np.random.RandomState(41))
    data[::7, 30:33, :] *= 6
    flag = flag.copy()
    flag[::7, 31, :] = True
    strategies = [{"task": "flag_autos"}, {"task": TASK, "kwargs": dict(KW, freq_chunks=2)}]
    with compared():
        whole, w_orig, w_final = scan.flag_scan(data, flag, ant1, ant2, tm, freq, width, strategies)
        chunked, c_orig, c_final = scan.flag_scan(data, flag, ant1, ant2, tm, freq, width, strategies, baseline_chunks=4)
        assert isinstance(whole, np.ndarray) and np.array_equal(whole, chunked)
        assert _plain(w_orig) == _plain(c_orig) and _plain(w_final) == _plain(c_final)
        base, _, _ = scan.flag_scan(data, flag, ant1, ant2, tm, freq, width, strategies[:1])
        assert (whole >= base).all() and (whole != base).any() and not whole.all()
        ds = dict(DATA=data, FLAG=flag, ANTENNA1=ant1, ANTENNA2=ant2, TIME=tm, CHAN_FREQ=freq, CHAN_WIDTH=width,
                  FIELD_ID=0, DATA_DESC_ID=0, SCAN_NUMBER=1)
        a, sa = scan.flag_scans([ds], strategies)
        b, sb = scan.flag_scans([ds], strategies, baseline_chunks=4)
        assert sa == sb and np.array_equal(np.asarray(a[0]), np.asarray(b[0])) and np.array_equal(np.asarray(a[0]), whole)


@pytest.mark.gpu
def test_gpu_every_listed_kernel_instantiation_was_launched_and_compared(gpu):
    """One compared call per route (the tests above add theirs when they ran): each launches exactly the instantiations
    its dtype and alignment select, and together they are the table."""
    vi = {"c64": 0, "f32": 1}
    for dtype in ("c64", "f32"):
        for offset in (False, True):
            vis, flags = make_case((2, 1, 10, 16), 110, 0.05, dtype)
            with compared() as log:
                check(("routes", dtype), vis, flags, dict(KW, freq_chunks=2), offset=offset)
            want = {"k_hyst_level<%d, 0>" % vi[dtype], "k_hyst_level<%d, 1>" % vi[dtype], "k_hyst_eligible<%d>" % vi[dtype],
                    "k_hyst_pack", "k_hyst_grow<%s>" % ("false" if offset else "true")}
            assert {k for k in log if k.startswith("k_hyst_")} == want, (dtype, offset, log)
    listed = set().union(*KERNELS.values())
    assert MET == listed, (sorted(listed - MET), sorted(MET - listed))
