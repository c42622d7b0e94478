"""Sliding 2-D median background and robust z-score flagging
(``median_filter_background``, ``median_zscore``, ``threshold_median_zscore``):
the NumPy restatement of the definition (``include/tricolour_amd.h``) against
a plain per-sample loop, the argument checks, the ABI and the behaviour on
noise with injected outliers on the CPU; the device kernel against the
restatement on the GPU.

No tolerance anywhere.  Both medians are exact selections, the mean of two
middle values, the subtraction and the quotient are single correctly rounded
operations: background, residual, scale, z-score and flags must agree in every
bit.  Every NaN of the definition is 0x7FC00000, in the restatement and on the
device alike, so NaN positions are compared by their bits as well.

This module also keeps the kernel table of ``tricolour_amd/csrc/steps/medz/``:
KERNELS lists every ``__global__`` kernel there with each instantiation a
launch site can produce; a CPU test holds it to the sources, and the last GPU
test shows with the library's kernel log that every listed instantiation was
launched by a call whose result was compared with the restatement."""
import contextlib
import ctypes as C
import glob
import os
import re
import warnings

import numpy as np
import pytest

from conftest import ROOT

NAN32 = np.uint32(0x7FC00000).view(np.float32)
MAD_NORMAL = 1.4826
TILE_ROWS, TILE_COLS = 16, 64       # MEDZ_TR, MEDZ_TC of kernels_medz.hpp: the tile of a block
ROWS_PER_THREAD = 4                 # MEDZ_PT

# every __global__ kernel of csrc/steps/medz/ and its instantiations, in the spelling of the kernel log
# (k_medz_select<VIS, RES>: VIS 0 = complex64, 1 = float32; RES: the keys come from the residual image)
KERNELS = {"k_medz_select": {"k_medz_select<0, false>", "k_medz_select<1, false>", "k_medz_select<1, true>"}}
MET = set()        # instantiations launched by calls whose results equalled the restatement


# ---------------------------------------------------------------------------
# the definition, restated
# ---------------------------------------------------------------------------
def amplitude(vis):
    """float32, +inf where a part is infinite."""
    vis = np.asarray(vis)
    if not np.iscomplexobj(vis):
        return np.abs(vis.astype(np.float32))
    re_, im = vis.real.astype(np.float64), vis.imag.astype(np.float64)
    with np.errstate(all="ignore"):
        a = np.sqrt(re_ * re_ + im * im).astype(np.float32)
    a[np.isinf(vis.real) | np.isinf(vis.imag)] = np.inf
    return a


def canonical(x):
    """float32 with every NaN as 0x7FC00000."""
    x = np.array(x, np.float32)
    x[np.isnan(x)] = NAN32
    return x


def default_min_samples(kt, kf):
    return max(1, ((2 * kt + 1) * (2 * kf + 1) + 7) // 8)


def sliding_median(x, kt, kf, min_samples):
    """The median rule over the truncated neighbourhoods of a (time, chan) float32 image whose NaNs do not count."""
    T, F = x.shape
    pad = np.pad(x.astype(np.float64), ((kt, kt), (kf, kf)), constant_values=np.nan)
    w = np.lib.stride_tricks.sliding_window_view(pad, (2 * kt + 1, 2 * kf + 1)).reshape(T, F, -1)
    n = (~np.isnan(w)).sum(-1)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        med = np.nanmedian(w, axis=-1)
    med[n < min_samples] = np.nan
    with np.errstate(over="ignore"):
        return canonical(med.astype(np.float32))


def restate_window(a, g, kt, kf, min_samples):
    """(background, residual, scale, z) of one (time, chan) amplitude image under the flags g."""
    valid = ~g & np.isfinite(a)
    b = sliding_median(np.where(valid, a, NAN32), kt, kf, min_samples)
    with np.errstate(all="ignore"):
        r = canonical(np.where(valid & ~np.isnan(b), a - b, NAN32))
    m, z = restate_scale(r, kt, kf, min_samples)
    return b, r, m, z


def restate_scale(r, kt, kf, min_samples):
    """(scale, z) of one residual image."""
    with np.errstate(all="ignore"):
        m = sliding_median(np.abs(r), kt, kf, min_samples)
        z = (r.astype(np.float64) / (m.astype(np.float64) * MAD_NORMAL)).astype(np.float32)
    z = canonical(np.where(~np.isnan(r) & ~np.isnan(m), z, NAN32))
    return m, z


def restate(vis, flags, kt, kf, min_samples=None, nsigma=6.0, rounds=1):
    """dict of background, residual, scale, z (all of the LAST round; background ... z of round 1 under "first") and
    out = g_rounds, for (..., time, chan) inputs."""
    ms = default_min_samples(kt, kf) if min_samples is None else min_samples
    a = amplitude(vis)
    g = np.asarray(flags) != 0
    lead = a.shape[:-2]
    parts = {k: np.empty(a.shape, np.float32) for k in ("background", "residual", "scale", "z")}
    first = {k: np.empty(a.shape, np.float32) for k in parts}
    out = g.copy()
    for w in np.ndindex(*lead):
        gw = g[w].copy()
        for k in range(rounds):
            vals = restate_window(a[w], gw, kt, kf, ms)
            with np.errstate(invalid="ignore"):
                hit = np.abs(vals[3]).astype(np.float64) > nsigma
            if k == 0:
                for name, v in zip(parts, vals):
                    first[name][w] = v
            gw = gw | hit
        for name, v in zip(parts, vals):
            parts[name][w] = v
        out[w] = gw
    return dict(parts, first=first, out=out)


def loop_median(values, min_samples):
    """The median rule, literally."""
    s = sorted(values)
    n = len(s)
    if n < min_samples:
        return NAN32
    if n % 2:
        return np.float32(s[(n - 1) // 2])
    with np.errstate(over="ignore"):
        return np.float32((np.float64(s[n // 2 - 1]) + np.float64(s[n // 2])) / 2.0)


def loop_window(a, g, kt, kf, ms, nsigma):
    """One round of the definition for one window, sample by sample."""
    T, F = a.shape
    valid = ~g & np.isfinite(a)

    def hood(t, f):
        return [(tt, ff) for tt in range(max(0, t - kt), min(T, t + kt + 1))
                for ff in range(max(0, f - kf), min(F, f + kf + 1))]
    b, r, m, z = (np.full((T, F), NAN32) for _ in range(4))
    hit = np.zeros((T, F), bool)
    for t in range(T):
        for f in range(F):
            b[t, f] = loop_median([a[p] for p in hood(t, f) if valid[p]], ms)
            if valid[t, f] and not np.isnan(b[t, f]):
                r[t, f] = np.float32(a[t, f] - b[t, f])
    for t in range(T):
        for f in range(F):
            m[t, f] = loop_median([np.float32(abs(r[p])) for p in hood(t, f) if not np.isnan(r[p])], ms)
            if not np.isnan(r[t, f]) and not np.isnan(m[t, f]):
                with np.errstate(all="ignore"):
                    q = np.float32(np.float64(r[t, f]) / (np.float64(m[t, f]) * MAD_NORMAL))
                z[t, f] = NAN32 if np.isnan(q) else q
                hit[t, f] = np.float64(abs(z[t, f])) > nsigma
    return b, r, m, z, hit


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    view = {8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize]
    return np.array_equal(a.view(view), b.view(view))


def differing(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def make_vis(shape, seed, dtype="c64"):
    """Rayleigh-distributed amplitudes with a slowly varying level."""
    rng = np.random.default_rng(seed)
    if dtype == "c64":
        vis = np.empty(shape, np.complex64)
        vis.real = rng.standard_normal(shape, dtype=np.float32)
        vis.imag = rng.standard_normal(shape, dtype=np.float32)
    else:
        vis = rng.rayleigh(1.0, shape).astype(np.float32)
        vis[rng.uniform(size=shape) < 0.5] *= np.float32(-1)      # float32 input: the sign is dropped
    vis *= (1 + 0.5 * np.sin(np.arange(shape[-1]) / 25.0)).astype(np.float32)
    return vis


def make_case(shape, seed, dtype="c64", content="noise"):
    """(vis, flags): `content` names what the image holds beyond Rayleigh noise with 3 % spikes."""
    rng = np.random.default_rng(seed + 1000)
    vis = make_vis(shape, seed, dtype)
    flags = np.zeros(shape, bool)
    spikes = rng.uniform(size=shape) < 0.03
    vis[spikes] *= np.float32(20)
    T, F = shape[-2:]
    if content == "ties":
        a = np.ceil(np.minimum(amplitude(vis), 3.9) * 2).astype(np.float32) / 2          # 8 levels: 0.5 ... 4
        vis = a.astype(vis.dtype)
    elif content == "flags30":
        flags = rng.uniform(size=shape) < 0.3
    elif content == "blocks":
        flags[..., : T // 2 + 1, : F // 2 + 1] = True                                     # larger than any neighbourhood
        flags[..., T - 1, F - 1] = True
    elif content == "all_flagged":
        flags[:] = True
    elif content == "constant":
        vis[:] = vis.reshape(-1)[0]
    elif content == "zeros":
        vis[:] = 0
    elif content == "nonfinite":
        flat, fl = vis.reshape(-1), flags.reshape(-1)
        pos = rng.choice(flat.size, size=min(flat.size, 10), replace=False)
        if dtype == "c64":
            values = [complex(np.nan, 1.0), complex(1.0, np.nan), complex(np.inf, 2.0), complex(2.0, -np.inf),
                      complex(np.inf, np.nan), complex(np.nan, np.nan), complex(-np.inf, np.inf), complex(np.inf, 1.0),
                      complex(3e38, 3e38), complex(np.nan, np.inf)]
        else:
            values = [np.nan, np.nan, np.inf, -np.inf, np.inf, np.nan, -np.inf, np.inf, 3.4e38, -3.4e38]
        for p, v in zip(pos, values):
            flat[p] = v
        fl[pos[-1]] = True
    else:
        assert content == "noise"
    return vis, flags


def behaviour_input():
    """48 x 160 Rayleigh amplitudes on a slowly varying level, 7 samples raised by 12: three alone, four in a run
    along time.  The seed is fixed."""
    rs = np.random.RandomState(3)
    a = (rs.rayleigh(1.0, (48, 160)) * (1 + 0.5 * np.sin(np.arange(160) / 25.0))).astype(np.float32)
    injected = np.zeros(a.shape, bool)
    for t, f in ((5, 17), (30, 90), (44, 150), (20, 60), (21, 60), (22, 60), (23, 60)):
        injected[t, f] = True
    a[injected] += np.float32(12)
    return a, injected


def rounds_input(dtype="f32"):
    """Two weak outliers beside a dense cluster of strong ones: the cluster lifts the first round's scale around them,
    and once it is flagged the second round finds them."""
    vis = make_vis((1, 1, 24, 40), 7, "f32")
    vis = np.abs(vis)
    vis[0, 0, 8:12, 10:13] = 400.0
    vis[0, 0, 10, 14] += 9.0
    vis[0, 0, 9, 9] += 9.0
    flags = np.zeros(vis.shape, bool)
    if dtype == "c64":
        vis = (vis * np.exp(1j * 0.7)).astype(np.complex64)
    return vis, flags


ROUNDS_KW = dict(radius_time=2, radius_freq=2, nsigma=6.0)


# ---------------------------------------------------------------------------
# CPU: the restatement, the argument checks, the ABI, the kernel table, the behaviour
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["c64", "f32"])
def test_restatement_equals_the_per_sample_loop(dtype):
    cases = 0
    for shape, radii in (((1, 1, 6, 9), [(1, 1), (2, 3), (0, 2), (3, 0), (8, 8)]), ((1, 1, 1, 1), [(1, 1)]),
                         ((1, 1, 5, 4), [(1, 2), (2, 0)])):
        for content in ("noise", "ties", "flags30", "blocks", "all_flagged", "constant", "zeros", "nonfinite"):
            vis, flags = make_case(shape, 11 + cases, dtype, content)
            for kt, kf in radii:
                for ms in (None, 1, 4):
                    area = (2 * kt + 1) * (2 * kf + 1)
                    if ms is not None and ms > area:
                        continue
                    got = restate(vis, flags, kt, kf, ms, nsigma=3.0)
                    use = default_min_samples(kt, kf) if ms is None else ms
                    b, r, m, z, hit = loop_window(amplitude(vis)[0, 0], flags[0, 0], kt, kf, use, 3.0)
                    for name, want in zip(("background", "residual", "scale", "z"), (b, r, m, z)):
                        assert same_bits(got[name][0, 0], want), (shape, content, kt, kf, ms, name)
                    assert np.array_equal(got["out"][0, 0], flags[0, 0] | hit), (shape, content, kt, kf, ms)
                    cases += 1
    assert cases > 100


def test_restatement_rounds_are_the_loop_of_single_rounds():
    vis, flags = rounds_input()
    g = flags
    seen = []
    for k in range(1, 4):
        g = restate(vis, g, 2, 2, nsigma=6.0)["out"]
        seen.append(g)
        assert np.array_equal(restate(vis, flags, 2, 2, nsigma=6.0, rounds=k)["out"], g)
    assert (seen[1] & ~seen[0]).any()          # the second round adds hits on this input


def test_python_argument_errors_come_before_any_device_work():
    from tricolour_amd import flagging
    vis = np.zeros((3, 1, 4, 8), np.complex64)
    flags = np.zeros((3, 1, 4, 8), bool)
    fns = (flagging.median_filter_background, flagging.median_zscore, flagging.threshold_median_zscore)
    for fn in fns:
        with pytest.raises(ValueError):
            fn(vis, flags[:, :, :3])                               # a shape mismatch
        with pytest.raises(ValueError):
            fn(vis[0], flags[0])                                   # not 4-D
        for bad in (np.zeros(vis.shape, np.float64), np.zeros(vis.shape, np.complex128), np.zeros(vis.shape, np.int32)):
            with pytest.raises(ValueError, match="complex64 or float32"):
                fn(bad, flags)                                     # a dtype that is not accepted
        for kw in (dict(radius_time=2.5), dict(radius_freq=1.5), dict(radius_time=True), dict(radius_freq=False),
                   dict(radius_time=-1), dict(radius_freq=-1), dict(radius_time=33), dict(radius_freq=33),
                   dict(radius_time="3"), dict(radius_time=float("nan")), dict(radius_time=0, radius_freq=0),
                   dict(radius_time=12, radius_freq=13), dict(radius_time=32, radius_freq=5),
                   dict(min_samples=0), dict(min_samples=17 * 17 + 1), dict(radius_time=1, radius_freq=1, min_samples=10),
                   dict(min_samples=2.5), dict(min_samples=True)):
            with pytest.raises(ValueError):
                fn(vis, flags, **kw)
    for kw in (dict(nsigma=0), dict(nsigma=-1.0), dict(nsigma=float("nan")), dict(nsigma="x"), dict(rounds=0),
               dict(rounds=5), dict(rounds=1.5), dict(rounds=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            flagging.threshold_median_zscore(vis, flags, **kw)
        with pytest.raises(ValueError, match=next(iter(kw))):
            flagging.check_median_zscore_kwargs(**kw)
    assert flagging.check_median_zscore_kwargs() == (6.0, 8, 8, 37, 1)
    assert flagging.check_median_zscore_kwargs(3, 12.0, 12, 625, 4) == (3.0, 12, 12, 625, 4)
    assert flagging.check_median_zscore_kwargs(radius_time=0, radius_freq=32) == (6.0, 0, 32, 9, 1)
    assert flagging.check_median_zscore_kwargs(radius_time=0, radius_freq=1) == (6.0, 0, 1, 1, 1)
    assert flagging.check_median_zscore_kwargs(radius_time=32, radius_freq=4)[3] == default_min_samples(32, 4)


def test_header_declares_and_the_binding_exports_the_entry_points():
    from tricolour_amd import _lib
    with open(os.path.join(ROOT, "include", "tricolour_amd.h")) as fh:
        hdr = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in ("tri_medfilt_background", "tri_medfilt_zscore", "tri_median_zscore_threshold"):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl, name
        assert "stream" in decl.group(1) and "workspace" not in decl.group(1), name
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().tri_version() >= 109
    for name in ("kernels_medz.hpp", "medz_host.hpp"):
        assert os.path.join(ROOT, "tricolour_amd", "csrc", "steps", "medz", name) in _lib.DEPENDS


def test_abi_rejects_bad_arguments_without_a_launch():
    from tricolour_amd import _lib
    lib = _lib.lib()
    buf = (C.c_uint8 * 32768)()
    base = C.addressof(buf)
    v, f, o, a, b = (base + 4096 * i for i in range(5))
    nan = float("nan")

    def bg(vis=v, dtype=_lib.TRI_VIS_C64, flags=f, n_win=2, ntime=4, nchan=8, kt=2, kf=3, ms=1, back=a, res=b):
        return lib.tri_medfilt_background(vis, dtype, flags, n_win, ntime, nchan, kt, kf, ms, back, res, None)

    def zs(res=v, n_win=2, ntime=4, nchan=8, kt=2, kf=3, ms=1, scale=a, z=b):
        return lib.tri_medfilt_zscore(res, n_win, ntime, nchan, kt, kf, ms, scale, z, None)

    def step(vis=v, dtype=_lib.TRI_VIS_C64, flags=f, out=o, n_win=2, ntime=4, nchan=8, kt=2, kf=3, ms=1, nsigma=6.0,
             rounds=1, res=a, z=b):
        return lib.tri_median_zscore_threshold(vis, dtype, flags, out, n_win, ntime, nchan, kt, kf, ms, nsigma, rounds,
                                               res, z, None)
    _lib.kernel_log_begin()
    try:
        for fn in (bg, zs, step):
            for kw in (dict(n_win=-1), dict(ntime=-1), dict(nchan=-1), dict(kt=-1), dict(kf=-1), dict(kt=33), dict(kf=33),
                       dict(kt=0, kf=0), dict(kt=12, kf=13), dict(kt=32, kf=5), dict(ms=0), dict(ms=36), dict(ms=-3)):
                assert fn(**kw) == _lib.TRI_EINVAL, (fn.__name__, kw)
            assert b"" != lib.tri_last_error()
            assert fn(n_win=0) == _lib.TRI_OK and fn(ntime=0) == _lib.TRI_OK and fn(nchan=0) == _lib.TRI_OK  # empty
            # more tiles than one launch holds, and a window too large to index
            assert fn(n_win=1 << 31, ntime=1, nchan=1) == _lib.TRI_EUNSUPPORTED
            assert fn(n_win=1 << 20, ntime=1 << 30, nchan=1 << 30) == _lib.TRI_EUNSUPPORTED
            assert fn(ntime=1 << 31) == _lib.TRI_EUNSUPPORTED
        for fn in (bg, step):
            for kw in (dict(vis=None), dict(flags=None)):
                assert fn(**kw) == _lib.TRI_EINVAL, (fn.__name__, kw)
            for dt in (_lib.TRI_VIS_C128, _lib.TRI_VIS_F64, 17, -1):
                assert fn(dtype=dt) == _lib.TRI_EUNSUPPORTED
            # a bad argument is named before a bad dtype
            assert fn(dtype=17, kt=33) == _lib.TRI_EINVAL
        for kw in (dict(back=None), dict(back=v + 8), dict(back=f), dict(res=v), dict(res=f + 4), dict(res=a + 252),
                   dict(back=b)):
            assert bg(**kw) == _lib.TRI_EINVAL, kw
        for kw in (dict(res=None), dict(z=None), dict(z=v + 4), dict(scale=v), dict(scale=b + 8), dict(z=a)):
            assert zs(**kw) == _lib.TRI_EINVAL, kw
        for kw in (dict(out=None), dict(res=None), dict(z=None), dict(nsigma=0.0), dict(nsigma=-1.0), dict(nsigma=nan),
                   dict(rounds=0), dict(rounds=5), dict(rounds=-1), dict(out=f), dict(out=f + 63), dict(out=v + 100),
                   dict(res=v + 8), dict(res=f), dict(res=o + 60), dict(z=a + 4), dict(z=o), dict(z=v), dict(z=f + 1)):
            assert step(**kw) == _lib.TRI_EINVAL, kw
    finally:
        log = _lib.kernel_log_end()
    assert log == {}, log


# ---- the kernel table against the sources ----
def scan_medz_kernels():
    found = set()
    paths = sorted(glob.glob(os.path.join(ROOT, "tricolour_amd", "csrc", "steps", "medz", "*")))
    assert paths
    for path in paths:
        with open(path, encoding="utf-8") as fh:
            found.update(re.findall(r"__global__[\s\S]{0,200}?\b(k_\w+)\s*\(", fh.read()))
    return found


def test_kernel_table_lists_what_the_sources_hold():
    from test_route_ledger import scan_instances, scan_kernels
    assert scan_medz_kernels() == set(KERNELS)
    assert not set(KERNELS) & scan_kernels()                   # the ledger keeps the kernels directly under csrc/
    sites = scan_instances()                                   # launch sites of the host code, macros expanded
    for kernel, instances in KERNELS.items():
        assert sites.get(kernel) == instances, kernel
    with open(os.path.join(ROOT, "tricolour_amd", "csrc", "tricolour_amd.hip"), encoding="utf-8") as fh:
        hip = fh.read()
    assert '#include "steps/medz/kernels_medz.hpp"' in hip and '#include "steps/medz/medz_host.hpp"' in hip
    with open(os.path.join(ROOT, "tricolour_amd", "csrc", "steps", "medz", "kernels_medz.hpp"), encoding="utf-8") as fh:
        text = fh.read()
    for name, value in (("MEDZ_TR", TILE_ROWS), ("MEDZ_TC", TILE_COLS), ("MEDZ_PT", ROWS_PER_THREAD)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name


@pytest.mark.parametrize("radii", [(8, 8), (0, 32), (2, 2)])
def test_behaviour_injected_outliers_are_hit_and_noise_is_not(radii):
    """Measured with this restatement (RandomState(3)): 7 of 7 injected samples hit for every radius pair, and 0, 2 and
    1 false hits of 7673 for (8, 8), (0, 32) and (2, 2); the cap of 0.2 % (15 samples) is a condition, not the figure."""
    a, injected = behaviour_input()
    assert a.shape == (48, 160) and injected.sum() == 7
    out = restate(a[None, None], np.zeros((1, 1) + a.shape, bool), *radii, nsigma=6.0, rounds=1)["out"][0, 0]
    false_hits = int((out & ~injected).sum())
    print("radii %s: %d of 7 hit, %d false hits of %d" % (radii, int(out[injected].sum()), false_hits, (~injected).sum()))
    assert out[injected].all()
    assert false_hits <= 0.002 * (~injected).sum()


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
    MET.update(k for k in log if k.startswith("k_medz_"))


def dev(torch, a, offset=False):
    """A device copy of `a`; offset: a contiguous view whose base lies one element past an aligned address."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        return t.cuda()
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    flat[1:] = t.reshape(-1).cuda()
    return flat[1:].view(t.shape)


_CACHE = {}


def expected(key, vis, flags, kw):
    """The restatement's dict; computed once per key and left unchanged."""
    if key not in _CACHE:
        e = restate(vis, flags, kw["radius_time"], kw["radius_freq"], kw.get("min_samples"), kw.get("nsigma", 6.0),
                    kw.get("rounds", 1))
        for v in list(e["first"].values()) + [v for k, v in e.items() if k != "first"]:
            v.setflags(write=False)
        _CACHE[key] = e
    return _CACHE[key]


def device_scale(torch, residual, kw):
    """(scale, z) of tri_medfilt_zscore for a residual image on the device."""
    from tricolour_amd import _lib
    kt, kf = kw["radius_time"], kw["radius_freq"]
    ms = kw.get("min_samples") or default_min_samples(kt, kf)
    res = residual.contiguous()
    scale, z = torch.empty_like(res), torch.empty_like(res)
    n_win = res.shape[0] * res.shape[1]
    _lib.check(_lib.lib().tri_medfilt_zscore(res.data_ptr(), n_win, res.shape[2], res.shape[3], kt, kf, ms,
                                             scale.data_ptr(), z.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return scale, z


def check(key, vis, flags, kw, container="tensor", offset=False, max_windows=None):
    """median_filter_background, median_zscore, tri_medfilt_zscore and threshold_median_zscore on the device against the
    restatement: the bits of background, residual, scale and z, the flags, the results' container and dtype, and the
    inputs unchanged."""
    import torch
    from tricolour_amd import flagging
    e = expected(key, vis, flags, kw)
    extra = {} if max_windows is None else dict(_max_windows=max_windows)
    radii = {k: v for k, v in kw.items() if k in ("radius_time", "radius_freq", "min_samples")}
    if container == "numpy":
        v, f = vis.copy(), flags.copy()
    else:
        v, f = dev(torch, vis, offset), dev(torch, flags, offset)
        if offset and vis.size:
            assert v.data_ptr() % 16 != 0
        f0 = f.clone()
    b, r = flagging.median_filter_background(v, f, **radii, **extra)
    z = flagging.median_zscore(v, f, **radii, **extra)
    out = flagging.threshold_median_zscore(v, f, **kw, **extra)
    if container == "numpy":
        assert all(isinstance(x, np.ndarray) for x in (b, r, z, out))
        assert out.dtype == flags.dtype and same_bits(v, vis) and np.array_equal(f, flags)
        scale, z2 = device_scale(torch, torch.from_numpy(r).cuda(), kw)
    else:
        assert all(x.is_cuda for x in (b, r, z, out))
        assert out.dtype == f.dtype and same_bits(v.cpu().numpy(), vis) and torch.equal(f, f0)
        scale, z2 = device_scale(torch, r, kw)
        b, r, z, out = (x.cpu().numpy() for x in (b, r, z, out))
    got = dict(background=b, residual=r, scale=scale.cpu().numpy(), z=z, z_abi=z2.cpu().numpy())
    for name, g in got.items():
        want = e["first"]["z" if name == "z_abi" else name]
        assert g.dtype == np.float32 and g.shape == want.shape, (key, name, g.shape, want.shape)
        assert differing(g, want) == 0, "%s: %d %s bit patterns differ" % (key, differing(g, want), name)
    nbad = int(((out != 0) != e["out"]).sum())
    assert out.shape == e["out"].shape and nbad == 0, "%s: %d flags differ" % (key, nbad)
    return e


RADII = [(1, 0), (0, 1), (2, 3), (0, 32), (32, 0), (4, 32), (12, 12)]
# one row and one channel beyond a block's tile, so that four blocks share a window; an odd number of rows that is one
# more than a multiple of a thread's rows with a channel count that is no multiple of 4, two windows and two correlations
SHAPES = [(1, 1, TILE_ROWS + 1, TILE_COLS + 1), (2, 2, 2 * ROWS_PER_THREAD + 1, TILE_COLS + 6)]


def kw_of(radii, **more):
    return dict(radius_time=radii[0], radius_freq=radii[1], nsigma=4.0, **more)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
def test_gpu_smallest_shapes(gpu, dtype):
    with compared():
        vis, flags = make_case((1, 1, 1, 1), 1, dtype)
        check(("1x1", dtype), vis, flags, kw_of((1, 1)))
        check(("1x1-ms2", dtype), vis, flags, kw_of((1, 1), min_samples=2))
        vis, flags = make_case((2, 1, 5, 7), 2, dtype, "flags30")
        check(("5x7", dtype), vis, flags, kw_of((8, 8)))                  # the neighbourhood exceeds the image


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("radii", RADII, ids=lambda r: "%dx%d" % r)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gpu_shapes_and_radii(gpu, shape, radii, dtype):
    vis, flags = make_case(shape, 20 + RADII.index(radii), dtype, "flags30" if radii[0] % 2 else "noise")
    with compared():
        check((shape, radii, dtype), vis, flags, kw_of(radii))


CONTENTS = ["noise", "ties", "flags30", "blocks", "all_flagged", "constant", "zeros", "nonfinite"]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("content", CONTENTS)
def test_gpu_contents(gpu, content, dtype):
    vis, flags = make_case(SHAPES[1], 40 + CONTENTS.index(content), dtype, content)
    with compared():
        for radii in ((2, 3), (1, 8)):
            e = check((content, radii, dtype), vis, flags, kw_of(radii))
            if content == "blocks":
                assert np.isnan(e["background"]).any() and not np.isnan(e["background"]).all()
            if content == "constant":
                assert np.isnan(e["z"]).all() and (e["scale"] == 0).all()
            if content == "all_flagged":
                assert np.isnan(e["background"]).all() and e["out"].all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
def test_gpu_min_samples_at_a_neighbourhoods_count_and_one_above(gpu, dtype):
    """No flags, radii (1, 1): a corner's neighbourhood holds 4 samples, an edge's 6, an inner one 9."""
    vis, flags = make_case((1, 2, 5, 7), 50, dtype)
    with compared():
        for ms, nans in ((4, 0), (5, 4), (6, 4), (7, 4 + 2 * 3 + 2 * 5), (9, 4 + 2 * 3 + 2 * 5)):
            e = check(("ms", ms, dtype), vis, flags, kw_of((1, 1), min_samples=ms))
            assert int(np.isnan(e["background"][0, 0]).sum()) == nans, ms


@pytest.mark.gpu
def test_gpu_windows_are_isolated(gpu):
    """The middle window is 1e6 times the others: the outer windows' outputs are what they are when passed alone."""
    import torch
    from tricolour_amd import flagging
    vis, flags = make_case((3, 1, TILE_ROWS + 3, 70), 60, "c64", "flags30")
    vis[1] *= np.float32(1e6)
    kw = kw_of((4, 32))
    with compared():
        e = check("isolated", vis, flags, kw)
        for w in (0, 2):
            alone = restate(vis[w:w + 1], flags[w:w + 1], 4, 32, nsigma=4.0)
            for name in ("background", "residual", "scale", "z", "out"):
                assert same_bits(alone[name][0], e[name][w]), (w, name)
            b, r = flagging.median_filter_background(dev(torch, vis[w:w + 1]), dev(torch, flags[w:w + 1]), 4, 32)
            assert same_bits(b.cpu().numpy()[0], e["background"][w]) and same_bits(r.cpu().numpy()[0], e["residual"][w])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
def test_gpu_rounds(gpu, dtype):
    vis, flags = rounds_input(dtype)
    with compared():
        outs = [check(("rounds", k, dtype), vis, flags, dict(ROUNDS_KW, rounds=k))["out"] for k in (1, 2, 3)]
    assert (outs[1] & ~outs[0]).any() and (outs[2] >= outs[1]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("container", ["numpy", "tensor"])
def test_gpu_containers(gpu, container, dtype):
    import torch
    from tricolour_amd import flagging
    vis, flags = make_case((2, 2, 9, 21), 70, dtype, "flags30")
    kw = kw_of((2, 3), rounds=2)
    with compared():
        e = check(("containers", dtype), vis, flags, kw, container=container)
        check(("containers", dtype), vis, flags, kw, container=container, offset=container == "tensor")
        # flags of another dtype come back in it
        f8 = flags.astype(np.uint8) * 3
        out = flagging.threshold_median_zscore(vis if container == "numpy" else dev(torch, vis),
                                               f8 if container == "numpy" else dev(torch, f8), **kw)
        assert out.dtype == (np.uint8 if container == "numpy" else torch.uint8)
        out = out if container == "numpy" else out.cpu().numpy()
        assert np.array_equal(out, e["out"].astype(np.uint8))


@pytest.mark.gpu
def test_gpu_batching_gives_the_same_result(gpu):
    vis, flags = make_case((3, 2, TILE_ROWS + 1, 36), 80, "c64", "flags30")
    kw = kw_of((2, 3), rounds=2)
    with compared():
        check("batch", vis, flags, kw)
        check("batch", vis, flags, kw, max_windows=1)
        check("batch", vis, flags, kw, max_windows=4)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
def test_gpu_prior_contents_of_the_outputs_do_not_matter(gpu, dtype):
    """Each C entry point twice, every output buffer full of 0xFF bytes and full of zeros before the call."""
    import torch
    from tricolour_amd import _lib
    lib = _lib.lib()
    vis, flags = make_case(SHAPES[1], 90, dtype, "flags30")
    kt, kf, ms, nsigma, rounds = 2, 3, 5, 4.0, 2
    e1 = restate(vis, flags, kt, kf, ms, nsigma, 1)
    e2 = restate(vis, flags, kt, kf, ms, nsigma, rounds)
    odd = np.array(e1["residual"])                      # a residual image as a caller may hand it over
    odd[0, 0, 1, 2], odd[0, 0, 3, 3], odd[0, 1, 0, 0] = np.inf, -np.inf, NAN32
    m_odd, z_odd = (np.stack([np.stack([restate_scale(odd[i, j], kt, kf, ms)[k] for j in range(odd.shape[1])])
                              for i in range(odd.shape[0])]) for k in (0, 1))
    v, f, res_in = dev(torch, vis), dev(torch, flags).view(torch.uint8), dev(torch, odd)
    code = _lib.TRI_VIS_C64 if dtype == "c64" else _lib.TRI_VIS_F32
    n_win, (T, F) = vis.shape[0] * vis.shape[1], vis.shape[2:]
    stream = torch.cuda.current_stream().cuda_stream
    with compared():
        for fill in (0xFF, 0x00):
            img = [torch.full((vis.size * 4,), fill, dtype=torch.uint8, device="cuda").view(torch.float32).view(vis.shape)
                   for _ in range(6)]
            out = torch.full(vis.shape, fill, dtype=torch.uint8, device="cuda")
            _lib.check(lib.tri_medfilt_background(v.data_ptr(), code, f.data_ptr(), n_win, T, F, kt, kf, ms,
                                                  img[0].data_ptr(), img[1].data_ptr(), stream))
            _lib.check(lib.tri_medfilt_zscore(res_in.data_ptr(), n_win, T, F, kt, kf, ms, img[2].data_ptr(),
                                              img[3].data_ptr(), stream))
            _lib.check(lib.tri_median_zscore_threshold(v.data_ptr(), code, f.data_ptr(), out.data_ptr(), n_win, T, F, kt,
                                                       kf, ms, nsigma, rounds, img[4].data_ptr(), img[5].data_ptr(), stream))
            got = [x.cpu().numpy() for x in img]
            for name, g, want in (("background", got[0], e1["background"]), ("residual", got[1], e1["residual"]),
                                  ("scale", got[2], m_odd), ("z", got[3], z_odd),
                                  ("last residual", got[4], e2["residual"]), ("last z", got[5], e2["z"])):
                assert differing(g, want) == 0, (fill, name, differing(g, want))
            assert np.array_equal(out.cpu().numpy(), e2["out"].astype(np.uint8)), fill
            # the optional outputs left out: the same bits in the others
            back = torch.full_like(img[0], float("nan"))
            z = torch.full_like(img[0], float("nan"))
            _lib.check(lib.tri_medfilt_background(v.data_ptr(), code, f.data_ptr(), n_win, T, F, kt, kf, ms,
                                                  back.data_ptr(), None, stream))
            _lib.check(lib.tri_medfilt_zscore(res_in.data_ptr(), n_win, T, F, kt, kf, ms, None, z.data_ptr(), stream))
            assert differing(back.cpu().numpy(), e1["background"]) == 0 and differing(z.cpu().numpy(), z_odd) == 0
    assert np.isinf(m_odd).any() or np.isinf(z_odd).any()


@pytest.mark.gpu
def test_gpu_behaviour_on_the_device(gpu):
    """The behaviour input of the CPU test on the device."""
    a, injected = behaviour_input()
    with compared():
        for radii in ((8, 8), (0, 32), (2, 2)):
            e = check(("behaviour", radii), a[None, None], np.zeros((1, 1) + a.shape, bool),
                      dict(radius_time=radii[0], radius_freq=radii[1], nsigma=6.0))
            assert e["out"][0, 0][injected].all()


@pytest.mark.gpu
def test_gpu_every_listed_kernel_instantiation_was_launched_and_compared(gpu):
    """One compared call per dtype (the tests above add theirs when they ran): each launches exactly the instantiations
    its dtype selects, and together they are the table."""
    vi = {"c64": 0, "f32": 1}
    for dtype in ("c64", "f32"):
        vis, flags = make_case((2, 1, 10, 16), 110, dtype, "flags30")
        with compared() as log:
            check(("routes", dtype), vis, flags, kw_of((2, 3)))
        want = {"k_medz_select<%d, false>" % vi[dtype], "k_medz_select<1, true>"}
        assert {k for k in log if k.startswith("k_medz_")} == want, (dtype, log)
    listed = set().union(*KERNELS.values())
    assert MET == listed, (sorted(listed - MET), sorted(MET - listed))
