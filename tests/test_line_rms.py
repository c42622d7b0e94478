"""Line-RMS thresholding of whole timesteps and channels: the NumPy restatement
of the definition (line sums by ``math.fsum``, correctly rounded), its checks
on the CPU, the argument checks and strategy plumbing, and the device kernels
against the restatement.

Tolerances, derived and not measured.  The only inexact quantity on the device
is a float64 sum of n non-negative terms in an order the kernel chooses: its
relative error is at most (n - 1) * 2^-53, so ``rms`` is compared at relative
tolerance 2 * n * 2^-53 with n the line length.  Flags must equal the
restatement's except on lines the restatement itself marks undecided
(``|dev - nsigma * sigma| <= 1e-9 * max(rms, med, nsigma * sigma)``); at most
1 line in 1000 of a case may be undecided, and ``test_no_undecided_lines``
asserts that the committed inputs have none, so the exception is never taken."""
import functools
import json
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden

U = 2.0 ** -53


# ---------------------------------------------------------------------------
# the definition, restated
# ---------------------------------------------------------------------------
def power(vis):
    vis = np.asarray(vis)
    if np.iscomplexobj(vis):
        re, im = vis.real.astype(np.float64), vis.imag.astype(np.float64)
        return re * re + im * im
    a = vis.astype(np.float64)
    return a * a


def restate_rms(vis, flags):
    """(rms_time (bl, corr, time), rms_chan (bl, corr, chan), n_time, n_chan); NaN for empty lines."""
    p = power(vis)
    ok = (np.asarray(flags) == 0) & ~np.isnan(p)
    p = np.where(ok, p, 0.0)
    nbl, ncorr, T, F = p.shape
    s_t = np.empty((nbl, ncorr, T))
    s_c = np.empty((nbl, ncorr, F))
    for b in range(nbl):
        for c in range(ncorr):
            w = p[b, c]
            s_t[b, c] = [math.fsum(r) for r in w.tolist()]
            s_c[b, c] = [math.fsum(r) for r in np.ascontiguousarray(w.T).tolist()]
    n_t, n_c = ok.sum(axis=3), ok.sum(axis=2)
    with np.errstate(invalid="ignore", divide="ignore"):
        rms_t = np.where(n_t > 0, np.sqrt(s_t / n_t), np.nan)
        rms_c = np.where(n_c > 0, np.sqrt(s_c / n_c), np.nan)
    return rms_t, rms_c, n_t, n_c


def decide_lines(rms, nsigma, flag_low):
    """One window, one axis: (bad, undecided) per line."""
    rms = np.asarray(rms, np.float64)
    bad = np.zeros(rms.shape, bool)
    und = np.zeros(rms.shape, bool)
    if not nsigma > 0:
        return bad, und
    usable = np.isfinite(rms)
    bad |= ~np.isnan(rms) & ~usable
    u = rms[usable]
    if u.size < 3:
        return bad, und
    med = np.median(u)
    sigma = 1.4826 * np.median(np.abs(u - med))
    if not sigma > 1e-9 * med:
        return bad, und
    thr = nsigma * sigma
    with np.errstate(invalid="ignore"):
        dev = rms - med
        a = np.abs(dev) if flag_low else dev
        bad |= usable & (a > thr)
        und = usable & (np.abs(a - thr) <= 1e-9 * np.maximum(np.maximum(rms, med), thr))
    return bad, und


def decide(rms_t, rms_c, nsigma_time, nsigma_freq, flag_low):
    bad_t, und_t = np.zeros(rms_t.shape, bool), np.zeros(rms_t.shape, bool)
    bad_c, und_c = np.zeros(rms_c.shape, bool), np.zeros(rms_c.shape, bool)
    for b in range(rms_t.shape[0]):
        for c in range(rms_t.shape[1]):
            bad_t[b, c], und_t[b, c] = decide_lines(rms_t[b, c], nsigma_time, flag_low)
            bad_c[b, c], und_c[b, c] = decide_lines(rms_c[b, c], nsigma_freq, flag_low)
    return bad_t, bad_c, und_t, und_c


def restate_threshold(vis, flags, nsigma_time=3.5, nsigma_freq=3.0, flag_low=True, rms=None):
    """(out flags, undecided mask over samples, number of undecided lines)."""
    rms_t, rms_c = rms if rms is not None else restate_rms(vis, flags)[:2]
    bad_t, bad_c, und_t, und_c = decide(rms_t, rms_c, nsigma_time, nsigma_freq, flag_low)
    out = (np.asarray(flags) != 0) | bad_t[..., :, None] | bad_c[..., None, :]
    und = und_t[..., :, None] | und_c[..., None, :]
    return out, und, int(und_t.sum() + und_c.sum())


# ---------------------------------------------------------------------------
# inputs: every GPU comparison draws from here, so that the CPU suite can check them all for undecided lines
# ---------------------------------------------------------------------------
SMALL_SHAPES = [(1, 1, 1, 1), (2, 1, 1, 37), (1, 3, 29, 1), (2, 2, 2, 13), (1, 2, 3, 65), (2, 1, 17, 30),
                (1, 2, 9, 100), (3, 1, 5, 18), (2, 2, 7, 2), (1, 1, 3, 3), (2, 1, 33, 48)]
DENSITIES = [0.0, 0.1, 0.5, 0.95]
# Both sides of everything the launcher switches on (line RMS routes):
#   power pass: 16-byte loads iff nchan % 4 == 0 (and aligned bases); tiles of 64 rows (64 | 65, a 36-tile line),
#               strips of 1024 channels (1024 | 1025, a 137-strip line)
#   apply pass: 16 flags per lane iff nchan % 16 == 0 (and aligned bases); 4096 | 4112 channels (one | two pieces of a row)
ROUTE_SHAPES = [(1, 2, 64, 40), (1, 2, 65, 40), (1, 1, 2300, 67), (1, 2, 130, 1024), (1, 2, 130, 1025),
                (1, 1, 5, 4096), (1, 1, 4, 4112), (1, 1, 5, 4100), (1, 1, 6, 4098), (1, 1, 2, 140000),
                (1, 1, 3, 65537)]
PATTERNS = ["boost_row", "boost_chan", "low_row", "flagged_lines", "nan", "inf", "identical_rows"]
STRUCT_SHAPE = (2, 2, 70, 300)
BENCH_SHAPE = (16, 4, 1024, 4096)
SKA_SHAPE = (1, 2, 512, 65536)


def make_case(shape, seed, density=0.1, dtype="c64", lines=True):
    """Unit-variance noise on a per-window level, a few boosted and attenuated rows and channels, random input flags."""
    rng = np.random.default_rng(seed)
    nbl, ncorr, T, F = shape
    if dtype == "c64":
        vis = np.empty(shape, np.complex64)
        vis.real = rng.standard_normal(shape, dtype=np.float32)
        vis.imag = rng.standard_normal(shape, dtype=np.float32)
    else:
        vis = np.abs(rng.standard_normal(shape, dtype=np.float32))
    vis *= rng.uniform(0.5, 20.0, size=(nbl, ncorr, 1, 1)).astype(np.float32)
    if lines:
        for b in range(nbl):
            for c in range(ncorr):
                for _ in range(max(1, T // 40)):
                    vis[b, c, rng.integers(T)] *= np.float32(rng.choice([0.4, 0.6, 1.5, 2.0, 3.0]))
                for _ in range(max(1, F // 60)):
                    vis[b, c, :, rng.integers(F)] *= np.float32(rng.choice([0.4, 0.6, 1.5, 2.0, 3.0]))
    flags = rng.uniform(size=shape) < density if density > 0 else np.zeros(shape, bool)
    return vis, flags


def make_structured(pattern):
    vis, flags = make_case(STRUCT_SHAPE, 77, density=0.05, lines=False)
    if pattern == "boost_row":
        vis[:, :, 31] *= 3
    elif pattern == "boost_chan":
        vis[..., 123] *= 3
    elif pattern == "low_row":
        vis[:, :, 12] *= np.float32(0.3)
    elif pattern == "flagged_lines":
        flags[:, :, 20] = True
        flags[..., 200] = True
        vis[:, :, 20] *= 50                   # flagged: must not be seen
    elif pattern == "nan":
        vis[0, 0, 5, 7] = np.nan
        vis[1, 1, 9, 11] = complex(1.0, np.nan)
        vis[0, 1, 40, :] = np.nan             # an empty row made of NaN samples
        flags[0, 0, 5, 7] = flags[1, 1, 9, 11] = False
        flags[0, 1, 40, :] = False
    elif pattern == "inf":
        vis[0, 0, 33, 44] = np.inf
        flags[0, 0, 33, 44] = False
        flags[0, 0, 33, 45] = False
    elif pattern == "identical_rows":
        vis[:] = vis[:, :, :1]
        flags[:] = False
    return vis, flags


def all_cases():
    """(id, maker) of every input the GPU comparisons use."""
    out = []
    for i, shape in enumerate(SMALL_SHAPES):
        for j, d in enumerate(DENSITIES):
            for dt in ("c64", "f32"):
                out.append((("small", shape, d, dt), functools.partial(make_case, shape, 1000 + 10 * i + j, d, dt)))
    for i, shape in enumerate(ROUTE_SHAPES):
        for dt in ("c64", "f32"):
            out.append((("route", shape, dt), functools.partial(make_case, shape, 2000 + i, 0.1, dt)))
    for p in PATTERNS:
        out.append((("struct", p), functools.partial(make_structured, p)))
    for dt in ("c64", "f32"):
        out.append((("bench", dt), functools.partial(make_case, BENCH_SHAPE, 3000, 0.1, dt)))
        out.append((("ska", dt), functools.partial(make_case, SKA_SHAPE, 3001, 0.1, dt)))
    out.append((("containers",), functools.partial(make_case, (2, 2, 33, 65), 3002, 0.2)))
    out.append((("batches",), functools.partial(make_case, (7, 3, 70, 1100), 3003, 0.1)))
    return out


CASES = dict(all_cases())
_RMS = {}


def case(key):
    """(vis, flags, restated (rms_time, rms_chan)); the rms of a case is computed once per process."""
    vis, flags = CASES[key]()
    if key not in _RMS:
        _RMS[key] = restate_rms(vis, flags)[:2]
    return vis, flags, _RMS[key]


KWARGS = [dict(), dict(flag_low=False), dict(nsigma_time=0.0), dict(nsigma_freq=0.0),
          dict(nsigma_time=2.5, nsigma_freq=4.0)]


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_restatement_matches_plain_loops():
    rs = np.random.RandomState(5)
    for trial in range(60):
        T, F = int(rs.randint(1, 12)), int(rs.randint(1, 12))
        cplx = trial % 2 == 0
        vis = rs.standard_normal((1, 1, T, F)).astype(np.float32)
        if cplx:
            vis = (vis + 1j * rs.standard_normal(vis.shape)).astype(np.complex64)
        if trial % 5 == 0:
            vis[0, 0, rs.randint(T), rs.randint(F)] = np.nan
        if T > 3:
            vis[0, 0, 1] *= 6
        flags = rs.uniform(size=vis.shape) < rs.uniform(0, 0.6)
        nst, nsf, low = [(3.5, 3.0, True), (2.0, 0.0, False), (1.0, 1.5, True)][trial % 3]
        # plain loops
        def line(samples):
            ps = []
            for v, f in samples:
                p = float(v.real) * float(v.real) + float(v.imag) * float(v.imag) if cplx else float(v) * float(v)
                if not f and p == p:
                    ps.append(p)
            return math.sqrt(math.fsum(ps) / len(ps)) if ps else float("nan")
        rt = [line([(vis[0, 0, t, c], flags[0, 0, t, c]) for c in range(F)]) for t in range(T)]
        rc = [line([(vis[0, 0, t, c], flags[0, 0, t, c]) for t in range(T)]) for c in range(F)]

        def bad_lines(r, nsigma):
            u = sorted(x for x in r if math.isfinite(x))
            out = [x == x and not math.isfinite(x) and nsigma > 0 for x in r]
            if nsigma > 0 and len(u) >= 3:
                mid = lambda s: s[len(s) // 2] if len(s) % 2 else (s[len(s) // 2 - 1] + s[len(s) // 2]) / 2   # noqa: E731
                med = mid(u)
                sigma = 1.4826 * mid(sorted(abs(x - med) for x in u))
                if sigma > 1e-9 * med:
                    for i, x in enumerate(r):
                        if math.isfinite(x):
                            d = x - med
                            out[i] = out[i] or ((abs(d) if low else d) > nsigma * sigma)
            return out
        bt, bc = bad_lines(rt, nst), bad_lines(rc, nsf)
        exp = np.array([[flags[0, 0, t, c] or bt[t] or bc[c] for c in range(F)] for t in range(T)])
        rms_t, rms_c, _, _ = restate_rms(vis, flags)
        assert np.array_equal(rms_t[0, 0], np.array(rt), equal_nan=True)
        assert np.array_equal(rms_c[0, 0], np.array(rc), equal_nan=True)
        got, _, _ = restate_threshold(vis, flags, nst, nsf, low)
        assert np.array_equal(got[0, 0], exp)


def test_restatement_flags_what_it_should():
    vis, flags, rms = case(("struct", "boost_row"))
    out, _, _ = restate_threshold(vis, flags, rms=rms)
    assert out[:, :, 31].all()
    vis, flags, rms = case(("struct", "low_row"))
    assert restate_threshold(vis, flags, rms=rms)[0][:, :, 12].all()
    assert not restate_threshold(vis, flags, flag_low=False, rms=rms)[0][:, :, 12].all()


def test_restatement_inert_cases():
    vis, flags = make_case((1, 1, 2, 50), 1, 0.0)
    vis[0, 0, 1] *= 100                                        # two time lines only: the time axis is inert
    out, _, _ = restate_threshold(vis, flags, nsigma_freq=0.0)
    assert not out.any()
    vis, flags, rms = case(("struct", "identical_rows"))       # constant rows: zero spread along time
    bad_t, _, _, _ = decide(rms[0], rms[1], 3.5, 3.0, True)
    assert not bad_t.any()
    vis, flags = make_case((1, 2, 8, 9), 2, 0.0)
    allf = np.ones(flags.shape, bool)
    out, und, n_und = restate_threshold(vis, allf)
    assert out.all() and n_und == 0
    rms_t, rms_c, n_t, n_c = restate_rms(vis, allf)
    assert np.isnan(rms_t).all() and np.isnan(rms_c).all() and not n_t.any() and not n_c.any()


def test_no_undecided_lines():
    """Every input the GPU tests compare on, under every keyword set they use: no line of the restatement is within
    1e-9 of its threshold, so device and restatement must agree on every flag."""
    lines = flagged = 0
    for key in CASES:
        vis, flags, rms = case(key)
        for kw in KWARGS:
            out, _, n_und = restate_threshold(vis, flags, rms=rms, **kw)
            assert n_und == 0, (key, kw)
        bad_t, bad_c, _, _ = decide(rms[0], rms[1], 3.5, 3.0, True)
        lines += bad_t.size + bad_c.size
        flagged += int(bad_t.sum() + bad_c.sum())
    assert flagged > 0 and lines > 100000


@pytest.mark.parametrize("kw", [dict(nsigma_time=-0.1), dict(nsigma_time=float("nan")), dict(nsigma_freq=-1.0),
                                dict(nsigma_freq=float("nan"))])
def test_bad_nsigma_raises_without_gpu(kw):
    from tricolour_amd import flagging
    with pytest.raises(ValueError):
        flagging.threshold_line_rms(np.zeros((1, 1, 4, 4), np.complex64), np.zeros((1, 1, 4, 4), bool), **kw)


@pytest.mark.parametrize("shape", [(4, 4), (1, 4, 4), (1, 1, 1, 4, 4)])
def test_non_4d_raises_without_gpu(shape):
    from tricolour_amd import flagging
    with pytest.raises(ValueError):
        flagging.threshold_line_rms(np.zeros(shape, np.complex64), np.zeros(shape, bool))
    with pytest.raises(ValueError):
        flagging.line_rms(np.zeros(shape, np.complex64), np.zeros(shape, bool))


def test_shape_mismatch_raises_without_gpu():
    from tricolour_amd import flagging
    vis = np.zeros((1, 1, 4, 4), np.complex64)
    with pytest.raises(ValueError):
        flagging.threshold_line_rms(vis, np.zeros((1, 1, 4, 5), bool))
    with pytest.raises(ValueError):
        flagging.line_rms(vis, np.zeros((1, 1, 5, 4), bool))


def test_header_declares_line_rms():
    hdr = open(os.path.join(ROOT, "include", "tricolour_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bsize_t\s+tri_line_rms_workspace_bytes\s*\(", hdr)
    assert re.search(r"\bint\s+tri_line_rms\s*\(", hdr)
    assert re.search(r"\bint\s+tri_line_rms_threshold\s*\(", hdr)


def test_workspace_bytes():
    from tricolour_amd import _lib
    lib = _lib.lib()
    assert lib.tri_line_rms_workspace_bytes(0, 8, 8) == 0
    assert lib.tri_line_rms_workspace_bytes(3, 0, 8) == 0
    assert lib.tri_line_rms_workspace_bytes(3, 8, 0) == 0
    one = lib.tri_line_rms_workspace_bytes(1, 1024, 4096)
    four = lib.tri_line_rms_workspace_bytes(4, 1024, 4096)
    assert 0 < one < four <= 4 * one
    assert one < 0.05 * 9 * 1024 * 4096          # partial sums are a few per cent of the window


def test_abi_rejects_bad_arguments_without_launch():
    import ctypes as C
    from tricolour_amd import _lib
    lib = _lib.lib()
    buf = (C.c_uint8 * 8192)()
    a, b, v = C.addressof(buf), C.addressof(buf) + 2048, C.addressof(buf) + 4096
    ws = (C.c_uint8 * 16)()

    def thr(vis=v, src=a, dst=b, dtype=_lib.TRI_VIS_C64, n_win=1, ntime=4, nchan=8, nt=3.5, nf=3.0, w=None, wb=0):
        return lib.tri_line_rms_threshold(vis, dtype, src, dst, n_win, ntime, nchan, nt, nf, 1, w, wb, None)

    def stat(vis=v, src=a, rt=b, rc=b + 512, dtype=_lib.TRI_VIS_C64, n_win=1, ntime=4, nchan=8, w=None, wb=0):
        return lib.tri_line_rms(vis, dtype, src, n_win, ntime, nchan, rt, rc, None, None, w, wb, None)
    assert thr(vis=None) == _lib.TRI_EINVAL
    assert thr(src=None) == _lib.TRI_EINVAL
    assert thr(dst=None) == _lib.TRI_EINVAL
    assert thr(ntime=-1) == _lib.TRI_EINVAL
    for ns in (-0.1, float("nan")):
        assert thr(nt=ns) == _lib.TRI_EINVAL
        assert thr(nf=ns) == _lib.TRI_EINVAL
    assert thr(dst=a + 4) == _lib.TRI_EINVAL                   # out overlaps flags
    assert thr(n_win=0) == _lib.TRI_OK                         # empty: no launch
    assert thr(nchan=0) == _lib.TRI_OK
    assert thr() == _lib.TRI_EWORKSPACE
    assert thr(w=C.addressof(ws), wb=16) == _lib.TRI_EWORKSPACE
    for dt in (_lib.TRI_VIS_C128, _lib.TRI_VIS_F64, 17):
        assert thr(dtype=dt) == _lib.TRI_EUNSUPPORTED
        assert stat(dtype=dt) == _lib.TRI_EUNSUPPORTED
    assert stat(vis=None) == _lib.TRI_EINVAL
    assert stat(src=None) == _lib.TRI_EINVAL
    assert stat(rt=None) == _lib.TRI_EINVAL
    assert stat(rc=None) == _lib.TRI_EINVAL
    assert stat(nchan=-2) == _lib.TRI_EINVAL
    assert stat(ntime=0) == _lib.TRI_OK
    assert stat() == _lib.TRI_EWORKSPACE


def test_check_strategies_accepts_the_task():
    from tricolour_amd import scan
    scan.check_strategies([{"task": "sum_threshold", "kwargs": {}},
                           {"task": "threshold_line_rms", "kwargs": {"nsigma_time": 3.5, "nsigma_freq": 3.0}}])
    assert "threshold_line_rms" in scan.VALID_TASKS
    with pytest.raises(ValueError) as e:
        scan.check_strategies([{"task": "threshold_lines"}])
    assert e.value.args == ("Task '%s' does not name a valid task", "threshold_lines")


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def _unaligned(torch, a):
    """A contiguous device copy of `a` whose base is one element past an aligned address."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    flat[1:] = t.reshape(-1).cuda()
    return flat[1:].view(t.shape)


def _rms_close(got, exp, n, what):
    assert got.shape == exp.shape and got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(exp)), what
    fin = np.isfinite(exp)
    assert np.array_equal(got[~fin & ~np.isnan(exp)], exp[~fin & ~np.isnan(exp)]), what
    err = np.abs(got[fin] - exp[fin])
    tol = 2 * n * U * np.abs(exp[fin])
    worst = float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0
    print("%s: rms error / tolerance = %.3g (n = %d)" % (what, worst, n))
    assert (err <= tol).all(), "%s: rms error is %.3g of the tolerance" % (what, worst)


def _check_case(key, kwargs=KWARGS, unaligned=False, stats=True):
    import torch
    from tricolour_amd import flagging
    vis, flags, rms = case(key)
    if unaligned:
        v, f = _unaligned(torch, vis), _unaligned(torch, flags)
        assert v.data_ptr() % 16 != 0 and f.data_ptr() % 4 != 0
    else:
        v, f = torch.from_numpy(vis).cuda(), torch.from_numpy(flags).cuda()
    if stats:
        rt, rc = flagging.line_rms(v, f)
        _rms_close(rt.cpu().numpy(), rms[0], vis.shape[3], "%s time" % (key,))
        _rms_close(rc.cpu().numpy(), rms[1], vis.shape[2], "%s chan" % (key,))
    nlines = rms[0].size + rms[1].size
    for kw in kwargs:
        got = flagging.threshold_line_rms(v, f, **kw).cpu().numpy()
        exp, und, n_und = restate_threshold(vis, flags, rms=rms, **kw)
        assert n_und * 1000 <= nlines, (key, kw, n_und)
        nbad = int(((got != exp) & ~und).sum())
        assert nbad == 0, "%d of %d flags differ (%s, %s)" % (nbad, exp.size, key, kw)
    return vis, flags, rms


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["c64", "f32"])
@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gpu_small_and_odd_shapes(gpu, shape, density, dt):
    from tricolour_amd import flagging
    import torch
    vis, flags, _ = _check_case(("small", shape, density, dt))
    _check_case(("small", shape, density, dt), unaligned=True)
    got = flagging.threshold_line_rms(torch.from_numpy(vis).cuda(), torch.from_numpy(flags).cuda(),
                                      nsigma_time=0, nsigma_freq=0)
    assert np.array_equal(got.cpu().numpy(), flags)           # both axes off: a normalising copy


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS)
def test_gpu_structured_inputs(gpu, pattern):
    import torch
    from tricolour_amd import flagging
    vis, flags, rms = _check_case(("struct", pattern))
    v, f = torch.from_numpy(vis).cuda(), torch.from_numpy(flags).cuda()
    out = flagging.threshold_line_rms(v, f).cpu().numpy()
    new = out & ~flags
    if pattern == "boost_row":
        assert out[:, :, 31].all()
    elif pattern == "boost_chan":
        assert out[..., 123].all()
    elif pattern == "low_row":
        assert out[:, :, 12].all()
        assert not flagging.threshold_line_rms(v, f, flag_low=False).cpu().numpy()[:, :, 12].all()
    elif pattern == "flagged_lines":
        rt, rc = (x.cpu().numpy() for x in flagging.line_rms(v, f))
        assert np.isnan(rt[:, :, 20]).all() and np.isnan(rc[..., 200]).all()
        assert np.isfinite(np.delete(rt, 20, axis=2)).all() and np.isfinite(np.delete(rc, 200, axis=2)).all()
        hidden = vis.copy()
        hidden[:, :, 20] = 0                                  # what a flagged sample holds changes nothing
        assert np.array_equal(flagging.threshold_line_rms(torch.from_numpy(hidden).cuda(), f).cpu().numpy(), out)
    elif pattern == "nan":
        rt, _ = flagging.line_rms(v, f)
        assert np.isnan(rt[0, 1, 40].item()) and not out[0, 1, 40].all()
    elif pattern == "inf":
        rt, rc = (x.cpu().numpy() for x in flagging.line_rms(v, f))
        assert np.isposinf(rt[0, 0, 33]) and np.isposinf(rc[0, 0, 44])
        assert out[0, 0, 33].all() and out[0, 0, :, 44].all()
        assert np.isfinite(rt).sum() == rt.size - 1 and np.isfinite(rc).sum() == rc.size - 1
        # the inf line is flagged even where its axis is otherwise inert (a huge nsigma flags nothing else)
        big = flagging.threshold_line_rms(v, f, nsigma_time=1e30, nsigma_freq=1e30).cpu().numpy()
        exp = flags.copy()
        exp[0, 0, 33] = True
        exp[0, 0, :, 44] = True
        assert np.array_equal(big, exp)
    elif pattern == "identical_rows":
        assert not new.all(axis=3).any()                      # no whole row: the time axis is inert


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["c64", "f32"])
@pytest.mark.parametrize("shape", ROUTE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gpu_route_switches(gpu, shape, dt):
    _check_case(("route", shape, dt))
    _check_case(("route", shape, dt), kwargs=KWARGS[:2], unaligned=True)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["c64", "f32"])
def test_gpu_benchmark_geometry(gpu, dt):
    """64 windows of 1024 x 4096, the benchmark's launch geometry."""
    vis, flags, rms = _check_case(("bench", dt), kwargs=KWARGS[:1])
    out, _, _ = restate_threshold(vis, flags, rms=rms)
    assert (out & ~flags).any()


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["c64", "f32"])
def test_gpu_ska_geometry(gpu, dt):
    """SKA-shaped windows of 512 x 65536: 65536 channel lines per window go through the select in global memory."""
    _check_case(("ska", dt), kwargs=KWARGS[:2])


@pytest.mark.gpu
def test_gpu_line_rms_is_reproducible_bit_for_bit(gpu):
    import torch
    from tricolour_amd import flagging
    vis, flags, rms = case(("batches",))
    v, f = torch.from_numpy(vis).cuda(), torch.from_numpy(flags).cuda()
    first = [x.cpu().numpy() for x in flagging.line_rms(v, f)]
    _rms_close(first[0], rms[0], vis.shape[3], "batches time")
    _rms_close(first[1], rms[1], vis.shape[2], "batches chan")
    for max_windows in (None, 1, 2, 5, 20):
        again = [x.cpu().numpy() for x in flagging.line_rms(v, f, _max_windows=max_windows)]
        for a, b in zip(first, again):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), max_windows
    # an unaligned copy takes the narrow loads: the same sums in the same order
    again = [x.cpu().numpy() for x in flagging.line_rms(_unaligned(torch, vis), _unaligned(torch, flags))]
    for a, b in zip(first, again):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["numpy_bool", "cuda_bool", "cuda_uint8"])
def test_gpu_containers(gpu, kind):
    import torch
    from tricolour_amd import flagging
    vis, flags, rms = case(("containers",))
    exp, _, n_und = restate_threshold(vis, flags, rms=rms)
    assert n_und == 0
    if kind == "numpy_bool":
        v, arg = vis.copy(), flags.copy()
    elif kind == "cuda_bool":
        v, arg = torch.from_numpy(vis).cuda(), torch.from_numpy(flags).cuda()
    else:
        v, arg = torch.from_numpy(vis).cuda(), torch.from_numpy(flags.astype(np.uint8) * 3).cuda()
    v0 = v.copy() if kind == "numpy_bool" else v.clone()
    before = arg.copy() if kind == "numpy_bool" else arg.clone()
    out = flagging.threshold_line_rms(v, arg)
    rt, rc = flagging.line_rms(v, arg)
    if kind == "numpy_bool":
        assert isinstance(out, np.ndarray) and out.dtype == np.bool_
        assert isinstance(rt, np.ndarray) and isinstance(rc, np.ndarray)
        assert np.array_equal(arg, before) and np.array_equal(v, v0)
        got = out
    else:
        assert torch.is_tensor(out) and out.is_cuda and rt.is_cuda and rc.is_cuda
        assert out.dtype == (torch.bool if kind == "cuda_bool" else torch.uint8)
        assert torch.equal(arg, before) and torch.equal(v, v0)
        got = out.cpu().numpy() != 0
        rt, rc = rt.cpu().numpy(), rc.cpu().numpy()
    assert rt.shape == vis.shape[:3] and rc.shape == vis.shape[:2] + vis.shape[3:]
    _rms_close(rt, rms[0], vis.shape[3], "containers time")
    assert got.shape == exp.shape and np.array_equal(got, exp)


@pytest.mark.gpu
def test_gpu_apply_strategies_sum_threshold_then_line_rms(gpu):
    import torch
    from tricolour_amd import flagging
    from tricolour_amd.strategies import apply_strategies
    rs = np.random.RandomState(4)
    shape = (3, 2, 64, 256)
    vis = (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(np.complex64)
    vis[..., 40:43] *= 10.0
    vis[:, :, 21] *= np.float32(1.6)              # one noisy timestep
    flags = rs.uniform(size=shape) < 0.02
    st_kw = dict(num_major_iterations=2, background_iterations=2)
    lr_kw = dict(nsigma_time=3.5, nsigma_freq=3.0)
    v, f = torch.from_numpy(vis).cuda(), torch.from_numpy(flags).cuda()
    got = apply_strategies([{"task": "sum_threshold", "kwargs": st_kw},
                            {"task": "threshold_line_rms", "kwargs": lr_kw}], f, v)
    st = flagging.sum_threshold_flagger(v, f, **st_kw) | f
    by_hand = flagging.threshold_line_rms(v, st, **lr_kw) | st
    assert torch.equal(got, by_hand)
    got, st = got.cpu().numpy(), st.cpu().numpy()
    assert (got >= st).all() and (got != st).any()            # the step adds flags here
    assert got[:, :, 21].all() and not st[:, :, 21].all()     # the noisy timestep goes as a whole
    exp, und, n_und = restate_threshold(vis, st, **lr_kw)
    assert n_und == 0 and np.array_equal(got, exp | st)


@pytest.mark.gpu
def test_gpu_flag_scan_with_line_rms_whole_and_chunked(gpu):
    from tricolour_amd import scan
    from test_scan_host import g15_rows
    d, _ = load_golden("G15_scan.npz")
    case_ = json.loads(str(d["cases"]))[0]
    strategies = json.loads(str(d["strategies"]))
    more = strategies + [{"task": "threshold_line_rms", "kwargs": {"nsigma_time": 3.5, "nsigma_freq": 3.0}}]
    r = g15_rows(d)
    scan_no, field_name, ddid = json.loads(str(d["call"]))

    def run(strats, chunks):
        flags, _, _ = scan.flag_scan(
            r["data"], r["flag"], r["ant1"], r["ant2"], r["time"], d["chan_freq"], d["chan_width"], strats,
            model=r["model"] if case_["model"] else None, flagging_strategy=case_["strategy"],
            corr_type=d["corr_type"], ignore_flags=case_["ignore_flags"], antenna_positions=d["antspos"],
            masked_channels=[d["masked_channels_" + case_["dilate"]]], antenna_names=list(d["antsnames"]),
            scan_no=scan_no, field_name=field_name, ddid=ddid, baseline_chunks=chunks)
        return flags
    whole = run(more, None)
    chunked = run(more, 3)
    assert np.array_equal(whole, chunked)
    base = run(strategies, None)
    assert (whole >= base).all() and (whole != base).any()
