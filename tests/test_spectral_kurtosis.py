"""Spectral-kurtosis flagging along time (``spectral_kurtosis``,
``spectral_kurtosis_bounds``, ``apply_spectral_kurtosis``,
``threshold_spectral_kurtosis``): the NumPy restatement of the definition
(``include/tricolour_amd.h``) against a literal loop in Python floats, the
default tables, the argument checks, the ABI and the behaviour on noise with
injected interference on the CPU; the device kernels against the restatement
on the GPU.

No tolerance anywhere.  The power, the two sums in their sequential order and
the estimator are single correctly rounded float64 operations in a fixed order:
``sk`` must agree in every bit -- every NaN of the definition is 0x7FC00000, in
the restatement and on the device alike -- and ``count`` and the flags exactly.

This module also keeps the kernel table of ``tricolour_amd/csrc/steps/sk/``:
KERNELS lists every ``__global__`` kernel there with each instantiation a
launch site can produce; a CPU test holds it to the sources, and the last GPU
test shows with the library's kernel log that every listed instantiation was
launched by a call whose result was compared with the restatement."""
import contextlib
import ctypes as C
import glob
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_median_zscore import NAN32, dev, differing, same_bits
import test_median_zscore as tmz

ROWS_AHEAD = 4          # SK_RB of kernels_sk.hpp: rows loaded ahead of their arithmetic
APPLY_ROWS = 16         # SK_AR: rows of a block one lane of the apply pass walks
MAX_BLOCK = 65536       # SK_MAX_BLOCK

# every __global__ kernel of csrc/steps/sk/ and its instantiations, in the spelling of the kernel log
# (k_sk_stats<VIS, VEC>: VIS 0 = complex64, 1 = float32, VEC: 4 channels per lane; k_sk_apply<VEC>: 16 flags per lane)
KERNELS = {"k_sk_stats": {"k_sk_stats<0, false>", "k_sk_stats<0, true>", "k_sk_stats<1, false>", "k_sk_stats<1, true>"},
           "k_sk_apply": {"k_sk_apply<false>", "k_sk_apply<true>"}}
MET = set()        # instantiations launched by calls whose results equalled the restatement


# ---------------------------------------------------------------------------
# the definition, restated
# ---------------------------------------------------------------------------
def default_min_samples(M):
    return max(2, M // 2)


def power(vis):
    """float64: re * re + im * im (both products exact), x * x for float32 input."""
    vis = np.asarray(vis)
    with np.errstate(all="ignore"):
        if np.iscomplexobj(vis):
            re_, im = vis.real.astype(np.float64), vis.imag.astype(np.float64)
            return re_ * re_ + im * im
        x = vis.astype(np.float64)
        return x * x


def bounds_restated(M, d=1.0, nsigma_low=4.0, nsigma_high=4.0):
    """The default tables, entry by entry."""
    lower, upper = np.full(M + 1, np.nan), np.full(M + 1, np.nan)
    for n in range(2, M + 1):
        sigma = math.sqrt(2.0 * d * (d + 1.0) * n * n / ((n - 1.0) * (n * d + 2.0) * (n * d + 3.0)))
        if nsigma_low is not None:
            lower[n] = math.exp(-nsigma_low * sigma)
        if nsigma_high is not None:
            upper[n] = math.exp(nsigma_high * sigma)
    return lower, upper


def restate_stats(vis, flags, M, d=1.0, min_samples=None):
    """(sk float32, count int32) of (..., time, chan) inputs: vectorised over everything but the rows of a block, which
    are walked in order with S1 = S1 + p."""
    ms = default_min_samples(M) if min_samples is None else min_samples
    p = power(vis)
    valid = (np.asarray(flags) == 0) & np.isfinite(p)
    T, F = p.shape[-2:]
    nb = -(-T // M)
    sk = np.empty(p.shape[:-2] + (nb, F), np.float32)
    cnt = np.empty(sk.shape, np.int32)
    for b in range(nb):
        n = np.zeros(p.shape[:-2] + (F,), np.int64)
        S1 = np.zeros(n.shape, np.float64)
        S2 = np.zeros(n.shape, np.float64)
        with np.errstate(all="ignore"):
            for t in range(b * M, min(T, (b + 1) * M)):
                v, pt = valid[..., t, :], p[..., t, :]
                n = n + v
                S1 = np.where(v, S1 + pt, S1)
                S2 = np.where(v, S2 + (pt * pt), S2)
            dn = n.astype(np.float64)
            den = S1 * S1
            q = (dn * S2) / den
            k = ((dn * d + 1.0) / (dn - 1.0)) * (q - 1.0)
            s = k.astype(np.float32)
        s[(n < ms) | ~(den > 0) | np.isnan(s)] = NAN32
        sk[..., b, :] = s
        cnt[..., b, :] = n
    return sk, cnt


def restate_apply(sk, count, flags, M, lower, upper):
    """out (bool) of the decision: a NaN on either side never hits, nor does a count outside [0, M]."""
    T = np.asarray(flags).shape[-2]
    inside = (count >= 0) & (count <= M)
    n = np.clip(count, 0, M)
    with np.errstate(invalid="ignore"):
        s = sk.astype(np.float64)
        hit = inside & ((s < np.asarray(lower)[n]) | (s > np.asarray(upper)[n]))
    return (np.asarray(flags) != 0) | np.repeat(hit, M, axis=-2)[..., :T, :], hit


def restate(vis, flags, M, d=1.0, min_samples=None, bounds=None, nsigma=(4.0, 4.0)):
    """dict of sk, count, hit (per cell), out and the tables used (the default tables are host NumPy by definition:
    the library's own function, held to bounds_restated by test_default_bounds)."""
    from tricolour_amd import flagging
    lower, upper = flagging.spectral_kurtosis_bounds(M, d, *nsigma) if bounds is None else bounds
    sk, cnt = restate_stats(vis, flags, M, d, min_samples)
    out, hit = restate_apply(sk, cnt, flags, M, lower, upper)
    return dict(sk=sk, count=cnt, hit=hit, out=out, lower=np.asarray(lower, np.float64), upper=np.asarray(upper, np.float64))


def loop_stats(vis, flags, M, d, ms):
    """The definition, literally: one (time, chan) window, one block and one channel at a time, in Python floats."""
    T, F = vis.shape
    nb = -(-T // M)
    sk, cnt = np.empty((nb, F), np.float32), np.empty((nb, F), np.int32)
    cplx = np.iscomplexobj(vis)
    for b in range(nb):
        for c in range(F):
            n, S1, S2 = 0, 0.0, 0.0
            for t in range(b * M, min(T, (b + 1) * M)):
                if cplx:
                    re_, im = float(vis[t, c].real), float(vis[t, c].imag)
                    p = re_ * re_ + im * im
                else:
                    x = float(vis[t, c])
                    p = x * x
                if flags[t, c] == 0 and math.isfinite(p):
                    n += 1
                    S1 = S1 + p
                    S2 = S2 + (p * p)
            den = S1 * S1
            s = NAN32
            if n >= ms and den > 0.0:
                q = (float(n) * S2) / den
                k = ((float(n) * d + 1.0) / (float(n) - 1.0)) * (q - 1.0)
                with np.errstate(over="ignore"):
                    s = np.float32(k)
                if np.isnan(s):
                    s = NAN32
            sk[b, c], cnt[b, c] = s, n
    return sk, cnt


def loop_apply(sk, cnt, flags, M, lower, upper):
    T, F = flags.shape
    out = np.zeros((T, F), bool)
    for t in range(T):
        for c in range(F):
            s, n = float(sk[t // M, c]), int(cnt[t // M, c])
            hit = 0 <= n <= M and (s < float(lower[n]) or s > float(upper[n]))
            out[t, c] = flags[t, c] != 0 or hit
    return out


def pairwise(a):
    """Tree sum over axis 0."""
    return a[0] if len(a) == 1 else pairwise(a[:len(a) // 2]) + pairwise(a[len(a) // 2:])


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
CONTENTS = ["noise", "flags30", "blocks", "all_flagged", "constant", "zeros", "nonfinite", "huge", "tiny", "wide", "steady"]


def noise(rng, shape, dtype):
    if dtype == "c64":
        vis = np.empty(shape, np.complex64)
        vis.real = rng.standard_normal(shape, dtype=np.float32)
        vis.imag = rng.standard_normal(shape, dtype=np.float32)
        return vis
    return rng.standard_normal(shape, dtype=np.float32)


def make_case(shape, seed, dtype="c64", content="noise", M=4, min_samples=None):
    """(vis, flags): `content` names what the windows hold."""
    rng = np.random.default_rng(seed)
    vis = noise(rng, shape, dtype)
    flags = np.zeros(shape, bool)
    T, F = shape[-2:]
    if content == "flags30":
        flags = rng.uniform(size=shape) < 0.3
    elif content == "blocks":
        # per block, by channel: the whole block flagged, exactly min_samples valid rows, and one fewer
        ms = default_min_samples(M) if min_samples is None else min_samples
        for b in range(-(-T // M)):
            rows = min(T, (b + 1) * M) - b * M
            for c in range(F):
                keep = (0, ms, ms - 1)[c % 3] if F >= 3 else (ms, ms - 1)[c % 2]
                flags[..., b * M: b * M + max(0, rows - keep), c] = True
    elif content == "all_flagged":
        flags[:] = True
    elif content == "constant":
        vis[:] = vis.reshape(-1)[0]
    elif content == "zeros":
        vis[:] = 0
    elif content == "nonfinite":
        vis, flags = tmz.make_case(shape, seed, dtype, "nonfinite")      # its complex and real value lists
    elif content == "huge":                                             # amplitudes near 3e38: p * p near 1e154
        vis = (vis / np.abs(vis) * rng.uniform(2.0e38, 3.3e38, shape).astype(np.float32) * np.float32(0.7)).astype(vis.dtype)
    elif content == "tiny":                                             # subnormal parts
        vis = (vis * np.float32(1e-39)).astype(vis.dtype)
    elif content == "wide":                                             # amplitudes log-uniform over [1e-6, 1e6]
        vis = (vis / np.abs(vis) * (10.0 ** rng.uniform(-6, 6, shape)).astype(np.float32)).astype(vis.dtype)
    elif content == "steady":                                           # a carrier with a relative scatter of 3e-5
        vis = (vis / np.abs(vis) * (1 + 3e-5 * rng.standard_normal(shape)).astype(np.float32)).astype(vis.dtype)
    else:
        assert content == "noise"
    return vis, flags


def behaviour_input():
    """256 x 160 complex Gaussian noise on a slowly varying level with three injections; block_time 64.  The seed is
    fixed.  Returns (vis, the 7 injected cells as a (4, 160) mask, the 2 carrier cells)."""
    rs = np.random.RandomState(3)
    T, F, M = 256, 160, 64
    vis = (rs.standard_normal((T, F)) + 1j * rs.standard_normal((T, F))).astype(np.complex64) \
        * (1 + 0.5 * np.sin(np.arange(F) / 25)).astype(np.float32)
    vis[::10, 17] += 6                                  # pulsed, in all four blocks
    vis[64:192, 90] += 4 * np.exp(0.3j)                 # a steady carrier in blocks 1 and 2
    vis[200:203, 140] += 8                              # one burst in block 3
    injected = np.zeros((T // M, F), bool)
    injected[:, 17] = True
    injected[1:3, 90] = True
    injected[3, 140] = True
    carrier = np.zeros_like(injected)
    carrier[1:3, 90] = True
    return vis.astype(np.complex64), injected, carrier


# ---------------------------------------------------------------------------
# CPU: the restatement, the tables, the argument checks, the ABI, the kernel table, the behaviour
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["c64", "f32"])
def test_restatement_equals_the_literal_loop(dtype):
    cases = 0
    for shape in ((1, 1, 9, 7), (1, 1, 1, 1), (1, 1, 5, 4)):
        for content in CONTENTS:
            for M in (2, 3, 4, 9, 16):
                for ms, d in ((None, 1.0), (2, 2.0), (M, 0.5)):
                    vis, flags = make_case(shape, 11 + cases, dtype, content, M, ms)
                    use = default_min_samples(M) if ms is None else ms
                    got = restate(vis, flags, M, d, ms, nsigma=(3.0, 3.0))
                    sk, cnt = loop_stats(vis[0, 0], flags[0, 0], M, d, use)
                    assert same_bits(got["sk"][0, 0], sk), (shape, content, M, ms)
                    assert np.array_equal(got["count"][0, 0], cnt), (shape, content, M, ms)
                    out = loop_apply(sk, cnt, flags[0, 0], M, got["lower"], got["upper"])
                    assert np.array_equal(got["out"][0, 0], out), (shape, content, M, ms)
                    cases += 1
    assert cases > 100


def test_contents_reach_what_they_are_for():
    """The cases are what their names say: blocks at exactly min_samples and one below, NaN for zeros, large and
    subnormal values that stay finite, and inputs on which a pairwise sum is NOT the sequential one."""
    M = 16
    vis, flags = make_case((1, 1, 40, 9), 5, "c64", "blocks", M)
    e = restate(vis, flags, M)
    assert set(np.unique(e["count"][0, 0, :2])) == {0, 7, 8}
    assert not np.isnan(e["sk"][0, 0, 0, 1]) and np.isnan(e["sk"][0, 0, 0, 2]) and np.isnan(e["sk"][0, 0, 0, 0])
    # the short last block, 8 rows: it reaches min_samples = 8 when all are valid, and never min_samples = 9
    vis, flags = make_case((1, 1, 40, 9), 5, "c64", "noise", M)
    assert not np.isnan(restate(vis, flags, M)["sk"]).any()
    e = restate(vis, flags, M, min_samples=9)
    assert np.isnan(e["sk"][0, 0, 2]).all() and not np.isnan(e["sk"][0, 0, :2]).any() and not e["hit"][0, 0, 2].any()
    assert np.isnan(restate(*make_case((1, 1, 40, 9), 5, "c64", "zeros", M), M)["sk"]).all()
    for dtype in ("c64", "f32"):
        vis, flags = make_case((1, 1, 64, 9), 6, dtype, "huge", M)
        assert np.abs(vis).min() > 1e38 and (power(vis) ** 2 > 1e152).all()
        assert np.isfinite(restate(vis, flags, M)["sk"]).all()
        vis, flags = make_case((1, 1, 64, 9), 6, dtype, "tiny", M)
        assert 0 < np.abs(vis).max() < 1.1754944e-38           # every part is subnormal or zero
        # float64 holds the squared sum of squared float32 subnormals (>= 1e-180): no underflow, the values are regular
        assert np.isfinite(restate(vis, flags, M)["sk"]).all()
        vis, flags = make_case((1, 1, 64, 9), 6, dtype, "constant", M)
        assert (restate(vis, flags, M)["sk"] < 0.01).all()     # no scatter at all: far below any lower bound
    # the order of the sums: a pairwise sum of the wide-range input is not the sequential one, in float64; what of that
    # reaches the float32 sk is below its rounding there, so the steady input, whose q - 1 near 4e-9 cancels nine
    # digits, is the one on which another order changes the bits of sk itself
    for content, in_sk in (("wide", False), ("steady", True)):
        vis, flags = make_case((1, 1, 64, 33), 7, "c64", content, 64)
        p = power(vis)[0, 0]
        if content == "wide":
            assert p.min() < 1e-8 and p.max() > 1e8
        S1, S2 = np.zeros(33), np.zeros(33)
        for t in range(64):
            S1, S2 = S1 + p[t], S2 + (p[t] * p[t])
        T1, T2 = pairwise(p), pairwise(p * p)
        assert (S1 != T1).any() and (S2 != T2).any(), content
        estimate = lambda a, b: ((64.0 + 1.0) / (64.0 - 1.0) * ((64.0 * b) / (a * a) - 1.0)).astype(np.float32)
        seq = restate(vis, flags, 64)["sk"][0, 0, 0]
        assert differing(estimate(S1, S2), seq) == 0
        assert (differing(estimate(T1, T2), seq) > 0) == in_sk, content   # otherwise the case proves nothing


def test_default_bounds():
    from tricolour_amd import flagging
    for M in (2, 3, 16, 64, 256, 4096):
        for d in (1.0, 2.0, 0.5):
            lower, upper = flagging.spectral_kurtosis_bounds(M, d)
            assert lower.dtype == np.float64 and upper.dtype == np.float64 and lower.shape == upper.shape == (M + 1,)
            assert np.isnan(lower[:2]).all() and np.isnan(upper[:2]).all()
            assert (lower[2:] < 1).all() and (upper[2:] > 1).all() and (lower[2:] > 0).all()
            assert np.allclose(lower[2:] * upper[2:], 1.0, rtol=4 * np.finfo(np.float64).eps, atol=0)
            assert (np.diff(lower[4:]) > 0).all() and (np.diff(upper[4:]) < 0).all()      # monotone in n from 4 on
            want = bounds_restated(M, d)
            for got, w in zip((lower, upper), want):
                assert np.allclose(got[2:], w[2:], rtol=8 * np.finfo(np.float64).eps, atol=0)
    lower, upper = flagging.spectral_kurtosis_bounds(64, 1.0, None, 3.0)
    assert np.isnan(lower).all() and (upper[2:] > 1).all()
    lower, upper = flagging.spectral_kurtosis_bounds(64, 1.0, 3.0, None)
    assert np.isnan(upper).all() and (lower[2:] < 1).all()
    lo3, hi3 = flagging.spectral_kurtosis_bounds(64, 1.0, 3.0, 5.0)
    lo4, hi4 = flagging.spectral_kurtosis_bounds(64)
    assert (lo3[2:] > lo4[2:]).all() and (hi3[2:] > hi4[2:]).all()
    for kw in (dict(block_time=1), dict(block_time=MAX_BLOCK + 1), dict(block_time=2.5), dict(block_time=True),
               dict(shape=0.0), dict(shape=float("nan")), dict(nsigma_low=0.0), dict(nsigma_high=float("nan")),
               dict(nsigma_low=-1.0), dict(nsigma_high="x"), dict(nsigma_low=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            flagging.spectral_kurtosis_bounds(**dict(dict(block_time=64), **kw))


def test_python_argument_errors_come_before_any_device_work():
    from tricolour_amd import flagging
    vis = np.zeros((3, 1, 4, 8), np.complex64)
    flags = np.zeros((3, 1, 4, 8), bool)
    for fn in (flagging.spectral_kurtosis, flagging.threshold_spectral_kurtosis):
        with pytest.raises(ValueError):
            fn(vis, flags[:, :, :3])                               # a shape mismatch
        with pytest.raises(ValueError):
            fn(vis[0], flags[0])                                   # not 4-D
        for bad in (np.zeros(vis.shape, np.float64), np.zeros(vis.shape, np.complex128), np.zeros(vis.shape, np.int32)):
            with pytest.raises(ValueError, match="complex64 or float32"):
                fn(bad, flags)                                     # a dtype that is not accepted
        for kw in (dict(block_time=1), dict(block_time=0), dict(block_time=-4), dict(block_time=MAX_BLOCK + 1),
                   dict(block_time=2.5), dict(block_time=True), dict(block_time="8"), dict(block_time=float("nan")),
                   dict(block_time=None), dict(shape=0), dict(shape=-1.0), dict(shape=float("nan")),
                   dict(shape=float("inf")), dict(shape="x"), dict(shape=True), dict(shape=None),
                   dict(min_samples=1), dict(min_samples=0), dict(min_samples=65), dict(min_samples=2.5),
                   dict(min_samples=True), dict(min_samples=float("nan")), dict(min_samples=5, block_time=4)):
            with pytest.raises(ValueError, match=next(iter(kw))):
                fn(vis, flags, **kw)
            with pytest.raises(ValueError, match=next(iter(kw))):
                flagging.check_spectral_kurtosis_kwargs(**kw)
    for kw in (dict(nsigma_low=0), dict(nsigma_low=-1.0), dict(nsigma_high=float("nan")), dict(nsigma_high="x"),
               dict(nsigma_low=True), dict(nsigma_high=float("inf"))):
        with pytest.raises(ValueError, match=next(iter(kw))):
            flagging.threshold_spectral_kurtosis(vis, flags, **kw)
        with pytest.raises(ValueError, match=next(iter(kw))):
            flagging.check_spectral_kurtosis_kwargs(**kw)
    tables = flagging.spectral_kurtosis_bounds(4)
    for bad in ((tables[0],), tables[0], (tables[0][:-1], tables[1]), (tables[0], np.zeros(6)), (np.zeros((5, 1)),) * 2,
                ("ab", tables[1]), 3.0):
        with pytest.raises(ValueError, match="bounds"):
            flagging.threshold_spectral_kurtosis(vis, flags, block_time=4, bounds=bad)
        with pytest.raises(ValueError, match="bounds"):
            flagging.apply_spectral_kurtosis(np.zeros((3, 1, 1, 8), np.float32), np.zeros((3, 1, 1, 8), np.int32), flags, 4,
                                             bad)
    sk, cnt = np.zeros((3, 1, 2, 8), np.float32), np.zeros((3, 1, 2, 8), np.int32)
    tables2 = flagging.spectral_kurtosis_bounds(2)
    for args in ((sk[:, :, :1], cnt, flags, 2, tables2), (sk, cnt[..., :7], flags, 2, tables2),
                 (sk.astype(np.float64), cnt, flags, 2, tables2), (sk, cnt.astype(np.int64), flags, 2, tables2),
                 (sk, cnt, flags[0], 2, tables2), (sk, cnt, flags, 1, tables2), (sk, cnt, flags, 2.5, tables2),
                 (sk, cnt, flags, True, tables2), (sk, cnt, flags, 4, tables)):       # block_time 4: one block, not two
        with pytest.raises(ValueError):
            flagging.apply_spectral_kurtosis(*args)
    assert flagging.check_spectral_kurtosis_kwargs() == (64, 1.0, 32, 4.0, 4.0)
    assert flagging.check_spectral_kurtosis_kwargs(2) == (2, 1.0, 2, 4.0, 4.0)
    assert flagging.check_spectral_kurtosis_kwargs(3, 2, 3, None, 3) == (3, 2.0, 3, None, 3.0)
    assert flagging.check_spectral_kurtosis_kwargs(MAX_BLOCK, 0.5, None, 2.5, None) == (MAX_BLOCK, 0.5, MAX_BLOCK // 2, 2.5, None)


def test_header_declares_and_the_binding_exports_the_entry_points():
    from tricolour_amd import _lib
    with open(os.path.join(ROOT, "include", "tricolour_amd.h")) as fh:
        hdr = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in ("tri_sk_statistics", "tri_sk_apply", "tri_sk_threshold"):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl, name
        assert "stream" in decl.group(1) and "workspace" not in decl.group(1), name
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().tri_version() >= 111
    for name in ("kernels_sk.hpp", "sk_host.hpp"):
        assert os.path.join(ROOT, "tricolour_amd", "csrc", "steps", "sk", name) in _lib.DEPENDS


def test_abi_rejects_bad_arguments_without_a_launch():
    from tricolour_amd import _lib
    lib = _lib.lib()
    buf = (C.c_uint8 * 32768)()
    base = C.addressof(buf)
    v, f, o, s, c, lo, hi = (base + 4096 * i for i in range(7))
    nan, inf = float("nan"), float("inf")

    # 2 windows of 4 x 8, block_time 2: vis 512 bytes, flags and out 64, sk and count 128 each, a table 24
    def st(vis=v, dtype=_lib.TRI_VIS_C64, flags=f, n_win=2, ntime=4, nchan=8, M=2, shape=1.0, ms=2, sk=s, count=c):
        return lib.tri_sk_statistics(vis, dtype, flags, n_win, ntime, nchan, M, shape, ms, sk, count, None)

    def ap(sk=s, count=c, flags=f, out=o, n_win=2, ntime=4, nchan=8, M=2, lower=lo, upper=hi):
        return lib.tri_sk_apply(sk, count, flags, out, n_win, ntime, nchan, M, lower, upper, None)

    def th(vis=v, dtype=_lib.TRI_VIS_C64, flags=f, out=o, n_win=2, ntime=4, nchan=8, M=2, shape=1.0, ms=2, lower=lo,
           upper=hi, sk=s, count=c):
        return lib.tri_sk_threshold(vis, dtype, flags, out, n_win, ntime, nchan, M, shape, ms, lower, upper, sk, count, None)
    _lib.kernel_log_begin()
    try:
        for fn in (st, ap, th):
            for kw in (dict(n_win=-1), dict(ntime=-1), dict(nchan=-1), dict(M=1), dict(M=0), dict(M=-2),
                       dict(M=MAX_BLOCK + 1), dict(flags=None), dict(sk=None)):
                assert fn(**kw) == _lib.TRI_EINVAL, (fn.__name__, kw)
            assert b"" != lib.tri_last_error()
            assert fn(n_win=0) == _lib.TRI_OK and fn(ntime=0) == _lib.TRI_OK and fn(nchan=0) == _lib.TRI_OK  # empty
            # more cells than one launch holds, and a window too large to index
            assert fn(n_win=1 << 31, ntime=1, nchan=1) == _lib.TRI_EUNSUPPORTED
            assert b"pass fewer windows per call" in lib.tri_last_error()
            assert fn(n_win=1 << 20, ntime=1 << 30, nchan=1 << 30) == _lib.TRI_EUNSUPPORTED
            assert fn(ntime=1 << 31) == _lib.TRI_EUNSUPPORTED
            assert fn(n_win=1 << 12, ntime=1 << 30, nchan=1) == _lib.TRI_EUNSUPPORTED      # 2^29 blocks of rows a window
            assert fn(M=MAX_BLOCK, n_win=(1 << 19) + 1, ntime=1, nchan=1) == _lib.TRI_EUNSUPPORTED   # 2^12 row chunks
        for fn in (st, th):
            for kw in (dict(vis=None), dict(shape=0.0), dict(shape=-1.0), dict(shape=nan), dict(shape=inf), dict(ms=1),
                       dict(ms=3), dict(ms=0), dict(ms=-1), dict(M=16, ms=17)):
                assert fn(**kw) == _lib.TRI_EINVAL, (fn.__name__, kw)
            for dt in (_lib.TRI_VIS_C128, _lib.TRI_VIS_F64, 17, -1):
                assert fn(dtype=dt) == _lib.TRI_EUNSUPPORTED
            # a bad argument is named before a bad dtype, a bad dtype before an empty shape and before a shape limit
            assert fn(dtype=17, M=1) == _lib.TRI_EINVAL and fn(dtype=17, shape=nan) == _lib.TRI_EINVAL
            assert fn(dtype=17, n_win=0) == _lib.TRI_EUNSUPPORTED
        assert st(count=None, n_win=0) == _lib.TRI_OK              # count is optional in the statistics
        for kw in (dict(sk=v + 8), dict(sk=v + 508), dict(sk=f), dict(sk=f + 63), dict(count=v), dict(count=f + 60),
                   dict(count=s), dict(count=s + 124), dict(sk=c + 4)):
            assert st(**kw) == _lib.TRI_EINVAL, kw
        for kw in (dict(count=None), dict(out=None), dict(lower=None), dict(upper=None), dict(out=f), dict(out=f + 63),
                   dict(out=s + 127), dict(out=c), dict(out=lo + 23), dict(out=hi), dict(out=hi - 63)):
            assert ap(**kw) == _lib.TRI_EINVAL, kw
        for kw in (dict(count=None), dict(out=None), dict(lower=None), dict(upper=None), dict(out=f), dict(out=v + 511),
                   dict(out=lo + 8), dict(out=hi + 23), dict(sk=v), dict(sk=f + 32), dict(sk=lo), dict(sk=hi + 20),
                   dict(sk=o + 60), dict(count=v + 256), dict(count=f), dict(count=lo + 16), dict(count=hi), dict(count=o),
                   dict(count=s + 4), dict(sk=c + 124)):
            assert th(**kw) == _lib.TRI_EINVAL, kw
    finally:
        log = _lib.kernel_log_end()
    assert log == {}, log


# ---- the kernel table against the sources ----
def scan_sk_kernels():
    found = set()
    paths = sorted(glob.glob(os.path.join(ROOT, "tricolour_amd", "csrc", "steps", "sk", "*")))
    assert paths
    for path in paths:
        with open(path, encoding="utf-8") as fh:
            found.update(re.findall(r"__global__[\s\S]{0,200}?\b(k_\w+)\s*\(", fh.read()))
    return found


def test_kernel_table_lists_what_the_sources_hold():
    from test_route_ledger import scan_instances, scan_kernels
    assert scan_sk_kernels() == set(KERNELS)
    assert not set(KERNELS) & scan_kernels()                   # the ledger keeps the kernels directly under csrc/
    sites = scan_instances()                                   # launch sites of the host code, macros expanded
    for kernel, instances in KERNELS.items():
        assert sites.get(kernel) == instances, kernel
    with open(os.path.join(ROOT, "tricolour_amd", "csrc", "tricolour_amd.hip"), encoding="utf-8") as fh:
        hip = fh.read()
    assert '#include "steps/sk/kernels_sk.hpp"' in hip and '#include "steps/sk/sk_host.hpp"' in hip
    with open(os.path.join(ROOT, "tricolour_amd", "csrc", "steps", "sk", "kernels_sk.hpp"), encoding="utf-8") as fh:
        text = fh.read()
    for name, value in (("SK_RB", ROWS_AHEAD), ("SK_AR", APPLY_ROWS), ("SK_MAX_BLOCK", MAX_BLOCK), ("SK_NT", 256)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
    assert "__shared__" not in text and "atomic" not in text.replace("no atomics", "")


def test_behaviour_pulsed_and_steady_interference_are_hit_and_noise_is_not():
    """Measured with this restatement (RandomState(3), block_time 64, nsigma 3 on both sides): 7 of 7 injected cells
    hit -- the two carrier cells below `lower`, the other five above `upper` -- and 4 false hits of the 633 clean
    cells; the cap of 2 % (12 cells) is a condition, not the figure.  The amplitude detectors' blind spots: the pulsed
    channel's samples are 6 sigma bursts at 10 % duty, and the carrier is constant in time."""
    vis, injected, carrier = behaviour_input()
    assert vis.shape == (256, 160) and injected.sum() == 7 and carrier.sum() == 2
    e = restate(vis[None, None], np.zeros((1, 1) + vis.shape, bool), 64, nsigma=(3.0, 3.0))
    hit, sk = e["hit"][0, 0], e["sk"][0, 0].astype(np.float64)
    low, high = hit & (sk < e["lower"][64]), hit & (sk > e["upper"][64])
    false_hits = int((hit & ~injected).sum())
    print("%d of 7 hit (%d low, %d high), %d false hits of %d" % (hit[injected].sum(), (low & injected).sum(),
                                                                  (high & injected).sum(), false_hits, (~injected).sum()))
    assert hit[injected].all()
    assert low[carrier].all() and high[injected & ~carrier].all()
    assert false_hits <= 0.02 * (~injected).sum()
    assert np.array_equal(e["out"][0, 0], np.repeat(hit, 64, axis=0))


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
    MET.update(k for k in log if k.startswith("k_sk_"))


_CACHE = {}


def expected(key, vis, flags, M, kw):
    """The restatement's dict; computed once per key and left unchanged."""
    if key not in _CACHE:
        e = restate(vis, flags, M, kw.get("shape", 1.0), kw.get("min_samples"), kw.get("bounds"),
                    (kw.get("nsigma_low", 4.0), kw.get("nsigma_high", 4.0)))
        for v in e.values():
            v.setflags(write=False)
        _CACHE[key] = e
    return _CACHE[key]


def c_entry_points(torch, v, f8, M, d, ms, lower, upper, fill=None, with_count=True):
    """(sk, count) of tri_sk_statistics, out of tri_sk_apply on them and (out, sk, count) of tri_sk_threshold for
    device tensors; fill: the byte every output buffer holds before the call."""
    from tricolour_amd import _lib
    lib = _lib.lib()
    nbl, ncorr, T, F = v.shape
    n_win, nb = nbl * ncorr, -(-T // M)
    code = _lib.TRI_VIS_C64 if v.dtype == torch.complex64 else _lib.TRI_VIS_F32
    stream = torch.cuda.current_stream().cuda_stream

    def new(shape, dtype):
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        if fill is None:
            return torch.empty(shape, dtype=dtype, device="cuda")
        return torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda").view(dtype).view(shape)
    lo, hi = dev(torch, np.array(lower, np.float64)), dev(torch, np.array(upper, np.float64))
    cells = (nbl, ncorr, nb, F)
    sk1, cnt1 = new(cells, torch.float32), new(cells, torch.int32)
    _lib.check(lib.tri_sk_statistics(v.data_ptr(), code, f8.data_ptr(), n_win, T, F, M, d, ms, sk1.data_ptr(),
                                     cnt1.data_ptr() if with_count else None, stream))
    out2 = new(v.shape, torch.uint8)
    if with_count:
        _lib.check(lib.tri_sk_apply(sk1.data_ptr(), cnt1.data_ptr(), f8.data_ptr(), out2.data_ptr(), n_win, T, F, M,
                                    lo.data_ptr(), hi.data_ptr(), stream))
    out3, sk3, cnt3 = new(v.shape, torch.uint8), new(cells, torch.float32), new(cells, torch.int32)
    _lib.check(lib.tri_sk_threshold(v.data_ptr(), code, f8.data_ptr(), out3.data_ptr(), n_win, T, F, M, d, ms,
                                    lo.data_ptr(), hi.data_ptr(), sk3.data_ptr(), cnt3.data_ptr(), stream))
    return [x.cpu().numpy() for x in (sk1, cnt1, out2, out3, sk3, cnt3)]


def check(key, vis, flags, M, container="tensor", offset=False, max_windows=None, **kw):
    """spectral_kurtosis, apply_spectral_kurtosis, threshold_spectral_kurtosis and the three C entry points on the
    device against the restatement: the bits of sk, count and the flags exactly, the results' container and dtype, and
    the inputs unchanged."""
    import torch
    from tricolour_amd import flagging
    e = expected(key, vis, flags, M, kw)
    extra = {} if max_windows is None else dict(_max_windows=max_windows)
    stat_kw = {k: v for k, v in kw.items() if k in ("shape", "min_samples")}
    d, ms = kw.get("shape", 1.0), kw.get("min_samples") or default_min_samples(M)
    tables = (e["lower"], e["upper"])
    if container == "numpy":
        v, f = vis.copy(), flags.copy()
    else:
        v, f = dev(torch, vis, offset), dev(torch, flags, offset)
        if offset and vis.size:
            assert v.data_ptr() % 16 != 0 and f.data_ptr() % 4 != 0
        f0 = f.clone()
    sk, cnt = flagging.spectral_kurtosis(v, f, M, **stat_kw, **extra)
    out_a = flagging.apply_spectral_kurtosis(sk, cnt, f, M, tables, **extra)
    out_t = flagging.threshold_spectral_kurtosis(v, f, M, **kw, **extra)
    if container == "numpy":
        assert all(isinstance(x, np.ndarray) for x in (sk, cnt, out_a, out_t))
        assert out_a.dtype == flags.dtype and out_t.dtype == flags.dtype
        assert same_bits(v, vis) and np.array_equal(f, flags)
        vd, fd = dev(torch, vis), dev(torch, flags)
    else:
        assert all(x.is_cuda for x in (sk, cnt, out_a, out_t))
        assert out_a.dtype == f.dtype and out_t.dtype == f.dtype
        vd, fd = v, f
        sk, cnt, out_a, out_t = (x.cpu().numpy() for x in (sk, cnt, out_a, out_t))
    abi = c_entry_points(torch, vd, fd.view(torch.uint8), M, d, ms, *tables)
    if container != "numpy":
        assert same_bits(v.cpu().numpy(), vis) and torch.equal(f, f0)
    for name, g in (("sk", sk), ("sk of tri_sk_statistics", abi[0]), ("sk of tri_sk_threshold", abi[4])):
        assert g.dtype == np.float32 and g.shape == e["sk"].shape, (key, name, g.shape, e["sk"].shape)
        assert differing(g, e["sk"]) == 0, "%s: %d %s bit patterns differ" % (key, differing(g, e["sk"]), name)
    for name, g in (("count", cnt), ("count of tri_sk_statistics", abi[1]), ("count of tri_sk_threshold", abi[5])):
        assert g.dtype == np.int32 and np.array_equal(g, e["count"]), (key, name)
    for name, g in (("apply", out_a), ("threshold", out_t), ("tri_sk_apply", abi[2]), ("tri_sk_threshold", abi[3])):
        nbad = int(((g != 0) != e["out"]).sum())
        assert g.shape == e["out"].shape and nbad == 0, "%s: %d flags of %s differ" % (key, nbad, name)
        assert set(np.unique(g.astype(np.uint8))) <= {0, 1}
    return e


def kernels_of(log):
    return {k for k in log if k.startswith("k_sk_")}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
def test_gpu_smallest_shapes(gpu, dtype):
    with compared():
        vis, flags = make_case((1, 1, 1, 1), 1, dtype)
        e = check(("1x1", dtype), vis, flags, 2)                      # one short block: NaN, nothing hit
        assert np.isnan(e["sk"]).all() and not e["out"].any()
        vis, flags = make_case((2, 1, 5, 7), 2, dtype, "flags30")
        e = check(("5x7", dtype), vis, flags, 64)                     # the block exceeds the window
        assert np.isnan(e["sk"]).all() and np.array_equal(e["out"], flags)
        check(("5x7-ms2", dtype), vis, flags, 64, min_samples=2, nsigma_low=1.0, nsigma_high=1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("M", [2, 3, 16, 64])
def test_gpu_block_edges(gpu, M, dtype):
    with compared():
        for T in (M - 1, M, M + 1, 2 * M + 1):
            vis, flags = make_case((2, 1, T, 9), 10 + T, dtype, "flags30" if T % 2 else "noise", M)
            e = check(("edges", M, T, dtype), vis, flags, M, nsigma_low=2.0, nsigma_high=2.0)
            assert e["sk"].shape[2] == -(-T // M)


# an aligned tensor of these channel counts: (statistics VEC, apply VEC)
CHANNELS = {4 * 64 + 1: (False, False), 272: (True, True), 260: (True, False)}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("nchan", sorted(CHANNELS))
def test_gpu_channel_counts_pick_each_instantiation(gpu, nchan, dtype):
    vi = {"c64": 0, "f32": 1}[dtype]
    spell = lambda vec: "true" if vec else "false"
    M = 6                                                             # a full group of rows ahead and a tail of 2
    vis, flags = make_case((2, 1, 2 * M + 1, nchan), 30, dtype, "flags30", M)
    vec_s, vec_a = CHANNELS[nchan]
    with compared() as log:
        check(("chan", nchan, dtype), vis, flags, M, nsigma_low=2.0, nsigma_high=2.0)
    assert kernels_of(log) == {"k_sk_stats<%d, %s>" % (vi, spell(vec_s)), "k_sk_apply<%s>" % spell(vec_a)}, log
    if nchan == 272:
        # a view one element past an aligned base falls back to the scalar kernels and gives the same bits
        with compared() as log:
            check(("chan", nchan, dtype), vis, flags, M, offset=True, nsigma_low=2.0, nsigma_high=2.0)
        assert kernels_of(log) == {"k_sk_stats<%d, false>" % vi, "k_sk_apply<false>"}, log


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("content", CONTENTS)
def test_gpu_contents(gpu, content, dtype):
    M = 16
    with compared():
        for nchan in (21, 32):                                        # the scalar and the vector kernels
            vis, flags = make_case((2, 2, 2 * M + 5, nchan), 40 + CONTENTS.index(content), dtype, content, M)
            e = check((content, nchan, dtype), vis, flags, M, nsigma_low=3.0, nsigma_high=3.0)
            if content == "blocks":
                assert set(np.unique(e["count"][:, :, :2])) == {0, 7, 8}
                assert np.isnan(e["sk"]).any() and not np.isnan(e["sk"]).all()
            if content in ("all_flagged", "zeros"):
                assert np.isnan(e["sk"]).all() and np.array_equal(e["out"], flags)
            if content == "constant":
                assert e["hit"][:, :, :2].all()
            if content in ("huge", "tiny", "wide", "steady"):
                assert np.isfinite(e["sk"][:, :, :2]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
def test_gpu_shape_parameter_and_min_samples(gpu, dtype):
    """30 % flags, block_time 8: the counts of the cells spread around 5.6; min_samples at 2, at a cell's exact count,
    one above it and at block_time."""
    M = 8
    vis, flags = make_case((2, 1, 3 * M, 24), 50, dtype, "flags30", M)
    n0 = int(restate_stats(vis, flags, M)[1][0, 0, 0, 0])
    assert 2 <= n0 < M
    with compared():
        for d in (1.0, 2.0, 0.5):
            check(("shape", d, dtype), vis, flags, M, shape=d, nsigma_low=2.0, nsigma_high=2.0)
        for ms in (2, n0, n0 + 1, M):
            e = check(("ms", ms, dtype), vis, flags, M, min_samples=ms, nsigma_low=2.0, nsigma_high=2.0)
            assert np.isnan(e["sk"][0, 0, 0, 0]) == (ms > n0)
            assert np.array_equal(np.isnan(e["sk"]), e["count"] < ms)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
def test_gpu_user_tables(gpu, dtype):
    M = 8
    vis, flags = make_case((2, 1, 3 * M + 2, 32), 60, dtype, "flags30", M)
    nan, inf = np.full(M + 1, np.nan), np.full(M + 1, np.inf)
    with compared():
        for name, bounds in (("nan", (nan, nan)), ("inf", (-inf, inf))):
            e = check(("tables", name, dtype), vis, flags, M, bounds=bounds)
            assert np.array_equal(e["out"], flags) and not np.isnan(e["sk"]).all()          # identity
        e = check(("tables", "all", dtype), vis, flags, M, bounds=(inf, inf))
        assert np.array_equal(e["hit"], ~np.isnan(e["sk"])) and e["hit"].any() and not e["hit"].all()
        one_sided = (nan, np.where(np.arange(M + 1) >= 6, 1.0, np.nan))                      # by count: 6 and more
        e = check(("tables", "count", dtype), vis, flags, M, bounds=one_sided)
        assert not e["hit"][e["count"] < 6].any() and e["hit"].any()


@pytest.mark.gpu
def test_gpu_apply_ignores_counts_outside_the_tables(gpu):
    """tri_sk_apply takes any statistics back in: a count outside [0, block_time] never hits (and reads no table)."""
    import torch
    from tricolour_amd import flagging
    M = 4
    rng = np.random.default_rng(65)
    flags = rng.uniform(size=(2, 1, 9, 32)) < 0.2
    sk = rng.uniform(0, 2, (2, 1, 3, 32)).astype(np.float32)
    sk[0, 0, 0, :4] = (np.nan, np.inf, -np.inf, 0.0)
    cnt = rng.integers(-2, M + 3, sk.shape).astype(np.int32)
    cnt[1, 0, 2, :4] = (np.iinfo(np.int32).max, np.iinfo(np.int32).min, -1, M + 1)
    bounds = flagging.spectral_kurtosis_bounds(M, 1.0, 0.5, 0.5)
    want, hit = restate_apply(sk, cnt, flags, M, *bounds)
    assert hit.any() and not hit[(cnt < 0) | (cnt > M)].any()
    with compared():
        for width in (32, 31):                                        # 16 flags per lane, and one
            got = flagging.apply_spectral_kurtosis(dev(torch, sk[..., :width]), dev(torch, cnt[..., :width]),
                                                   dev(torch, flags[..., :width]), M, bounds)
            assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want[..., :width])


@pytest.mark.gpu
def test_gpu_windows_are_isolated(gpu):
    """The middle window is 1e6 times the others: the outer windows' outputs are what they are when passed alone."""
    import torch
    from tricolour_amd import flagging
    M = 40                                                             # two full chunks of rows and one of 8 per block
    vis, flags = make_case((3, 1, 2 * M + 3, 36), 70, "c64", "flags30", M)
    vis[1] *= np.float32(1e6)
    kw = dict(nsigma_low=2.0, nsigma_high=2.0)
    with compared():
        e = check("isolated", vis, flags, M, **kw)
        for w in (0, 2):
            alone = restate(vis[w:w + 1], flags[w:w + 1], M, nsigma=(2.0, 2.0))
            for name in ("sk", "count", "out"):
                assert same_bits(alone[name][0], e[name][w]), (w, name)
            sk, cnt = flagging.spectral_kurtosis(dev(torch, vis[w:w + 1]), dev(torch, flags[w:w + 1]), M)
            assert same_bits(sk.cpu().numpy()[0], e["sk"][w]) and np.array_equal(cnt.cpu().numpy()[0], e["count"][w])
            out = flagging.threshold_spectral_kurtosis(dev(torch, vis[w:w + 1]), dev(torch, flags[w:w + 1]), M, **kw)
            assert np.array_equal(out.cpu().numpy()[0], e["out"][w])


@pytest.mark.gpu
def test_gpu_batching_gives_the_same_result(gpu):
    M = 16
    vis, flags = make_case((3, 2, 2 * M + 1, 36), 80, "c64", "flags30", M)
    kw = dict(nsigma_low=2.0, nsigma_high=2.0)
    with compared():
        check("batch", vis, flags, M, **kw)
        check("batch", vis, flags, M, max_windows=1, **kw)
        check("batch", vis, flags, M, max_windows=4, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("container", ["numpy", "tensor"])
def test_gpu_containers(gpu, container, dtype):
    import torch
    from tricolour_amd import flagging
    M = 4
    vis, flags = make_case((2, 2, 9, 21), 90, dtype, "flags30", M)
    kw = dict(nsigma_low=1.5, nsigma_high=1.5)
    with compared():
        e = check(("containers", dtype), vis, flags, M, container=container, **kw)
        check(("containers", dtype), vis, flags, M, container=container, offset=container == "tensor", **kw)
        assert e["hit"].any()
        # flags of another dtype, with values other than 1, come back in it as 0 / 1
        f8 = flags.astype(np.uint8) * 3
        args = (vis, f8) if container == "numpy" else (dev(torch, vis), dev(torch, f8))
        out = flagging.threshold_spectral_kurtosis(*args, M, **kw)
        assert out.dtype == (np.uint8 if container == "numpy" else torch.uint8)
        assert np.array_equal(out if container == "numpy" else out.cpu().numpy(), e["out"].astype(np.uint8))
        sk, cnt = flagging.spectral_kurtosis(*args, M)
        out = flagging.apply_spectral_kurtosis(sk, cnt, args[1], M, (e["lower"], e["upper"]))
        assert out.dtype == (np.uint8 if container == "numpy" else torch.uint8)
        assert np.array_equal(out if container == "numpy" else out.cpu().numpy(), e["out"].astype(np.uint8))
        # non-contiguous inputs: a transposed view of (chan, time) storage
        vt, ft = np.ascontiguousarray(vis.swapaxes(2, 3)), np.ascontiguousarray(flags.swapaxes(2, 3))
        args = (vt, ft) if container == "numpy" else (dev(torch, vt), dev(torch, ft))
        args = tuple(a.swapaxes(2, 3) if container == "numpy" else a.transpose(2, 3) for a in args)
        out = flagging.threshold_spectral_kurtosis(*args, M, **kw)
        assert np.array_equal(out if container == "numpy" else out.cpu().numpy(), e["out"])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
def test_gpu_prior_contents_of_the_outputs_do_not_matter(gpu, dtype):
    """Each C entry point twice, every output buffer full of 0xFF bytes and full of zeros before the call; and the
    statistics without a count image."""
    import torch
    M, d, ms = 6, 2.0, 3
    with compared():
        for nchan in (48, 19):
            vis, flags = make_case((2, 1, 2 * M + 1, nchan), 100, dtype, "flags30", M)
            lower, upper = bounds_restated(M, d, 2.0, 2.0)
            e = restate(vis, flags, M, d, ms, (lower, upper))
            assert e["hit"].any() and np.isnan(e["sk"]).any()
            v, f = dev(torch, vis), dev(torch, flags).view(torch.uint8)
            for fill in (0xFF, 0x00):
                got = c_entry_points(torch, v, f, M, d, ms, lower, upper, fill=fill)
                for g in (got[0], got[4]):
                    assert differing(g, e["sk"]) == 0, (fill, nchan)
                for g in (got[1], got[5]):
                    assert np.array_equal(g, e["count"]), (fill, nchan)
                for g in (got[2], got[3]):
                    assert np.array_equal(g, e["out"].astype(np.uint8)), (fill, nchan)
                alone = c_entry_points(torch, v, f, M, d, ms, lower, upper, fill=fill, with_count=False)
                assert differing(alone[0], e["sk"]) == 0
                assert (alone[1].view(np.uint8) == fill).all()            # the count image was not touched


@pytest.mark.gpu
def test_gpu_behaviour_on_the_device(gpu):
    """The behaviour input of the CPU test on the device."""
    vis, injected, carrier = behaviour_input()
    with compared():
        e = check("behaviour", vis[None, None], np.zeros((1, 1) + vis.shape, bool), 64, nsigma_low=3.0, nsigma_high=3.0)
    assert e["hit"][0, 0][injected].all() and injected.sum() == 7


@pytest.mark.gpu
def test_gpu_every_listed_kernel_instantiation_was_launched_and_compared(gpu):
    """One compared call per dtype and route (the tests above add theirs when they ran): each launches exactly the
    instantiations its dtype, channel count and alignment select, and together they are the table."""
    vi = {"c64": 0, "f32": 1}
    for dtype in ("c64", "f32"):
        for nchan, offset, want in ((32, False, {"k_sk_stats<%d, true>", "k_sk_apply<true>"}),
                                    (20, False, {"k_sk_stats<%d, true>", "k_sk_apply<false>"}),
                                    (32, True, {"k_sk_stats<%d, false>", "k_sk_apply<false>"})):
            vis, flags = make_case((2, 1, 10, nchan), 110, dtype, "flags30", 4)
            with compared() as log:
                check(("routes", dtype, nchan), vis, flags, 4, offset=offset, nsigma_low=2.0, nsigma_high=2.0)
            assert kernels_of(log) == {k % vi[dtype] if "%d" in k else k for k in want}, (dtype, nchan, offset, log)
    listed = set().union(*KERNELS.values())
    assert MET == listed, (sorted(listed - MET), sorted(MET - listed))
