"""Every kernel behind tri_uvcontsub_flagger against a host reference, stage by stage.

tri_uvcontsub_flagger_debug taps the last major cycle of a call: the time-mean spectrum (k_uv_mean), its low-passed form
(k_uv_lowpass), the residual and the flags the MAD ignores (k_uv_resid / k_uv_resid4), the two medians (the eight
k_medbig_* instantiations, the second one with the centred key | |x| - m |), the flagged count, and the returned flags
(k_uv_apply / k_uv_apply4).  Each stage is compared with a plain numpy reference of that stage alone, fed with the
device's own input to it, so a stage's rounding never excuses the next one:

    mean       bit for bit with the device's rule restated (float32 sums in time order, one float64 division), which is
               itself held to the float64 mean of the same samples by the bound of sequential float32 summation
    low pass   within a derived bound of a direct DFT in long double of the tapped mean
    residual   bit for bit (oracle.abs_c64 of the float32 difference), the MAD mask and the flagged count exactly
    medians    bit for bit (numba's median rule, tests/test_gpu_parity.py::_np_median_abs)
    decision   exactly

The fixture `proof` runs every case of CASES once, each between kernel_log_begin() and kernel_log_end(); the kernels of a
log count as met only if the case passed every stage check.  The last GPU test asserts that all fourteen instantiations
(six k_uv_*, k_medbig_range, k_medbig_pick and both forms of k_medbig_hist, _compact and _select) were met and nothing
else but k_normalise_flags was launched.  The tests at the end need no device: the references against each other and,
composed into a whole cycle, against oracle.uvcontsub_flagger.
"""
import traceback
import warnings

import numpy as np
import pytest

from test_gpu_parity import _np_median_abs
from test_route_ledger import UV_CLOSING, matches, reachable_instances

gpu_only = pytest.mark.gpu

SIGMA = 5.1          # (not a float32 number: the device must round it once, as the decision reference does)
L = np.longdouble
PI_L = L(4) * np.arctan(L(1))

# The float64 part of the low-pass bound, per component of smooth[f], in units of 2^-53 * mean|avg|.  The device forms
# K bins X[k] = sum_f avg[f] e^{-2 pi i k f / F} and smooth[f] = (1 / F) sum_k X[k] e^{+2 pi i k f / F} in float64.
# To first order a sum of F products carries an error of at most F u sum_f |avg[f]| (u = 2^-53; the twiddle's own
# rounding adds a term of the same form with a small constant instead of F), so |dX[k]| <~ F u (F mean|avg|); the
# inverse adds K such errors divided by F, and its own K-term sum adds K u |X| / F <= K u mean|avg| per term: together
# (K F + K K + c K) u mean|avg| <= 4 K F u mean|avg| with K <= F (a component of a complex product sees |re| + |im|
# <= sqrt(2) |avg|, which the factor also covers).  The final rounding to float32 adds half a float32 ulp of the result.
LOWPASS_F64_FACTOR = 4.0


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
def _general(rs, T, F):
    x = np.linspace(0, 1, F)
    vis = ((2 + np.cos(7 * x))[None, :] + 0.3 * rs.standard_normal((T, F))
           + 1j * (0.5 * x[None, :] + 0.3 * rs.standard_normal((T, F)))).astype(np.complex64)
    vis[rs.uniform(size=(T, F)) < 0.03] += 4
    flags = (rs.uniform(size=(T, F)) < 0.05).astype(np.uint8)
    N = T * F
    if F >= 3:
        flags[:, F // 2] = 1                         # a fully flagged channel
    if N >= 6:
        fl = flags.reshape(-1)
        fl[1], fl[N - 2] = 2, 255                    # flag bytes other than 0 / 1
        i = N // 3 + (1 if (N // 3) % F == F // 2 else 0)
        vis.reshape(-1)[i] = np.nan                  # an unflagged NaN
        fl[i] = 0
    if N == 1:
        flags[:] = 0
    return vis, flags


def _product(kind, rs, T, F):
    N = T * F
    vis, flags = _general(rs, T, F)
    if kind == "general":
        pass
    elif kind == "allflag":
        flags = np.array([1, 2, 255], np.uint8)[rs.randint(0, 3, size=(T, F))]
    elif kind == "one":                               # one unflagged sample
        flags[:] = 1
        flags[T // 2, F // 3] = 0
        vis[T // 2, F // 3] = 1.5 - 0.25j
    elif kind == "const":                             # constant visibilities: mad == 0
        vis[:] = 2 - 1j
        flags = (rs.uniform(size=(T, F)) < 0.05).astype(np.uint8) if N > 1 else np.zeros((T, F), np.uint8)
    elif kind == "tie":
        # constant but for four unflagged zeros, one in each lane of a group of four samples.  With taylor_degrees = 0
        # the residual is |vis|: mad == 0, the threshold is 0 and the zeros sit exactly on it.  `>` leaves them
        # unflagged and flags every other sample; `>=` would flag them too.
        vis[:] = 2 - 1j
        flags = (rs.uniform(size=(T, F)) < 0.05).astype(np.uint8)
        vis.reshape(-1)[N // 2:N // 2 + 4] = 0
        flags.reshape(-1)[N // 2:N // 2 + 4] = 0
    elif kind == "nanonly":                           # the only unflagged samples are NaN, in either component
        flags[:] = 1
        for i, z in ((0, complex(np.nan, 1.0)), (N - 1, complex(1.0, np.nan)))[:N]:
            vis.reshape(-1)[i] = z
            flags.reshape(-1)[i] = 0
    elif kind == "inf1":                              # a single unflagged +Inf (in the last channel: the mean's last block)
        vis[T // 2, F - 1] = complex(np.inf, 0.25)
        flags[T // 2, F - 1] = 0
    elif kind == "infpm":                             # +Inf and -Inf in one channel
        f = F - 1
        vis[0, f], vis[1, f] = complex(np.inf, 0.5), complex(-np.inf, 0.5)
        flags[0, f] = flags[1, f] = 0
    elif kind == "wide":                              # amplitudes over 30 binary orders of magnitude
        amp = np.exp2(rs.permutation(np.linspace(-15, 15, N))).reshape(T, F)
        vis = (amp * np.exp(2j * np.pi * rs.uniform(size=(T, F)))).astype(np.complex64)
    elif kind == "overfill":
        # With taylor_degrees = 0 the residual is |vis|: 20000 samples at 1, 20000 at 3, half of the rest below 1 and
        # half above 3 (30 binary orders in all).  The median is 2 and | |x| - 2 | equals 1 for 40000 samples: more equal
        # keys around the second median than the candidate list of the centred select holds (32768).
        assert N % 2 == 0 and N > 40000
        rest = (N - 40000) // 2
        amp = np.concatenate([np.ones(20000), np.full(20000, 3.0), np.exp2(rs.uniform(-15, -0.01, rest)),
                              4 * np.exp2(rs.uniform(0, 13, rest))]).astype(np.float32)
        amp = amp[rs.permutation(N)].reshape(T, F)
        vis = np.where(rs.uniform(size=(T, F)) < 0.5, amp + 0j, 1j * amp).astype(np.complex64)
        flags = np.zeros((T, F), np.uint8)
    else:
        raise KeyError(kind)
    return vis, flags


def make_inputs(shape, kinds, seed):
    n, T, F = shape
    assert len(kinds) == n
    rs = np.random.RandomState(seed)
    pairs = [_product(k, rs, T, F) for k in kinds]
    return (np.ascontiguousarray(np.stack([p[0] for p in pairs])), np.ascontiguousarray(np.stack([p[1] for p in pairs])))


def _case(shape, kinds, taylor, or_from, cycles=1, variant="plain"):
    return dict(shape=shape, kinds=kinds, taylor=taylor, or_from=or_from, cycles=cycles, variant=variant)


# name -> (n_cp, ntime, nchan), one data kind per product, taylor_degrees, or_original_from_cycle, major_cycles, call variant.
# Constant products go with taylor_degrees = 0 and single-sample products with taylor_degrees < nchan: there mad == 0 and
# the threshold is 0, so that the comparison with the oracle (whose FFT rounds differently) stays decidable.  Every shape,
# and each of the two call variants, carries every kind it can hold (kinds_a_shape_can_hold).
CASES = {
    "1x1x1": _case((1, 1, 1), ["general"], 20, 0),
    "1x1x1-K0": _case((1, 1, 1), ["const"], 0, 0),
    "1x1x1-K1-replace": _case((1, 1, 1), ["allflag"], 1, 1),
    "1x1x1-K20-nan": _case((1, 1, 1), ["nanonly"], 20, 0),
    "2x3x5-K20-replace": _case((2, 3, 5), ["general", "allflag"], 20, 1),              # K = nchan: smooth == avg
    "2x3x5-K1": _case((2, 3, 5), ["inf1", "nanonly"], 1, 0),
    "2x3x5-K1-wide": _case((2, 3, 5), ["infpm", "wide"], 1, 0),
    "2x3x5-K0": _case((2, 3, 5), ["const", "one"], 0, 0),
    "2x3x5-K0-tie": _case((2, 3, 5), ["tie", "general"], 0, 0),
    "3x7x260-K20": _case((3, 7, 260), ["general", "inf1", "infpm"], 20, 0),
    "3x7x260-K64-replace": _case((3, 7, 260), ["wide", "allflag", "one"], 64, 1),
    "3x7x260-K1-three cycles": _case((3, 7, 260), ["general", "one", "nanonly"], 1, 1, cycles=3),
    "3x7x260-K0": _case((3, 7, 260), ["const", "tie", "wide"], 0, 0),
    "3x7x260-K20-offset base": _case((3, 7, 260), ["general", "inf1", "infpm"], 20, 0, variant="offset"),
    "3x7x260-K1-offset base-replace": _case((3, 7, 260), ["one", "nanonly", "wide"], 1, 1, variant="offset"),
    "3x7x260-K0-offset base": _case((3, 7, 260), ["const", "tie", "allflag"], 0, 0, variant="offset"),
    "5x7x260-K20-batches of 2": _case((5, 7, 260), ["general", "inf1", "infpm", "allflag", "one"], 20, 0, variant="batched"),
    "5x7x260-K0-batches of 2": _case((5, 7, 260), ["const", "tie", "nanonly", "wide", "one"], 0, 0, variant="batched"),
    "2x5x258-K20": _case((2, 5, 258), ["general", "infpm"], 20, 0),
    "2x5x258-K64": _case((2, 5, 258), ["inf1", "wide"], 64, 0),
    "2x5x258-K1-replace": _case((2, 5, 258), ["allflag", "nanonly"], 1, 1),
    "2x5x258-K0": _case((2, 5, 258), ["const", "one"], 0, 0),
    "2x5x258-K0-tie": _case((2, 5, 258), ["tie", "general"], 0, 0),
    "2x6x258-K20": _case((2, 6, 258), ["general", "inf1"], 20, 1),
    "2x6x258-K64": _case((2, 6, 258), ["infpm", "wide"], 64, 0),
    "2x6x258-K1": _case((2, 6, 258), ["allflag", "nanonly"], 1, 0),
    "2x6x258-K0": _case((2, 6, 258), ["const", "one"], 0, 0),
    "2x6x258-K0-tie": _case((2, 6, 258), ["tie", "general"], 0, 0),
    "2x33x2050-K0": _case((2, 33, 2050), ["wide", "const"], 0, 0),
    "2x33x2050-K20": _case((2, 33, 2050), ["general", "inf1"], 20, 0),
    "2x33x2050-K64": _case((2, 33, 2050), ["infpm", "one"], 64, 0),
    "2x33x2050-K1-replace": _case((2, 33, 2050), ["allflag", "nanonly"], 1, 1),
    "2x33x2050-K0-tie": _case((2, 33, 2050), ["tie", "general"], 0, 0),
    "2x32x2052-K0": _case((2, 32, 2052), ["overfill", "const"], 0, 0),
    "2x32x2052-K64": _case((2, 32, 2052), ["general", "wide"], 64, 0),
    "2x32x2052-K20": _case((2, 32, 2052), ["inf1", "infpm"], 20, 0),
    "2x32x2052-K1-replace": _case((2, 32, 2052), ["allflag", "nanonly"], 1, 1),
    "2x32x2052-K0-tie": _case((2, 32, 2052), ["tie", "one"], 0, 0),
}

KINDS = {"general", "allflag", "one", "const", "tie", "nanonly", "inf1", "infpm", "wide", "overfill"}


def kinds_a_shape_can_hold(shape):
    """A single sample is the one-sample product already, cannot sit on a threshold beside others, span a range, or be
    infinite with a finite median beside it; only (2, 32, 2052) is cut for the overfilled candidate list."""
    n, T, F = shape
    if T * F == 1:
        return {"general", "allflag", "const", "nanonly"}
    return KINDS - (set() if shape == (2, 32, 2052) else {"overfill"})


_INPUTS = {}


def inputs(name):
    if name not in _INPUTS:
        c = CASES[name]
        vis, flags = make_inputs(c["shape"], c["kinds"], 100 + sorted(CASES).index(name))
        vis.setflags(write=False)
        flags.setflags(write=False)
        _INPUTS[name] = (vis, flags)
    return _INPUTS[name]


def infinite_samples(vis):
    return np.isinf(vis.real) | np.isinf(vis.imag)


# ---------------------------------------------------------------------------
# host references, one per stage
# ---------------------------------------------------------------------------
def ref_mean(vis, start, zero_nonfinite=True):
    """The device's rule: float32 sums in time order over the samples that are neither flagged nor NaN in either
    component, float32(float64(sum) / float64(n)); 0 where nothing counted or (the reference's isnan reset through
    numpy's complex division) where a sum is not finite.  Returns (avg complex64, n, sum_re, sum_im)."""
    n_cp, T, F = vis.shape
    ok = ~start & ~np.isnan(vis.real) & ~np.isnan(vis.imag)
    sr, si = np.zeros((n_cp, F), np.float32), np.zeros((n_cp, F), np.float32)
    with np.errstate(all="ignore"):
        for t in range(T):
            sr = np.where(ok[:, t], sr + vis.real[:, t], sr)
            si = np.where(ok[:, t], si + vis.imag[:, t], si)
        assert sr.dtype == np.float32 and si.dtype == np.float32
        n = ok.sum(axis=1)
        keep = n > 0
        if zero_nonfinite:
            keep &= np.isfinite(sr) & np.isfinite(si)
        d = np.maximum(n, 1).astype(np.float64)
        avg = np.zeros((n_cp, F), np.complex64)
        avg.real = np.where(keep, (sr.astype(np.float64) / d).astype(np.float32), np.float32(0))
        avg.imag = np.where(keep, (si.astype(np.float64) / d).astype(np.float32), np.float32(0))
    return avg, n, sr, si


def half_ulp32(x):
    """Half a float32 ulp at |x| (x of any float type): the most that rounding x to float32 can change it."""
    x = np.abs(np.asarray(x, np.float64))
    _, e = np.frexp(x)                                         # |x| in [2^(e-1), 2^e); subnormal spacing below 2^-126
    return np.ldexp(0.5, np.where(x == 0, -149, np.maximum(e - 24, -149)))


def mean_bound_errors(vis, start):
    """ref_mean against the float64 mean of the same samples: (n - 1) 2^-24 sum|x| for the sequential float32 sum, over n,
    plus half a float32 ulp of the result.  Channels with a non-finite sum are left out (their average is 0 by rule)."""
    avg, n, sr, si = ref_mean(vis, start)
    ok = ~start & ~np.isnan(vis.real) & ~np.isnan(vis.imag)
    out = []
    for part, s32, a in (("re", sr, avg.real), ("im", si, avg.imag)):
        x = np.where(ok, getattr(vis, "real" if part == "re" else "imag"), 0).astype(np.float64)
        with np.errstate(all="ignore"):
            s64, sabs = x.sum(axis=1), np.abs(x).sum(axis=1)
            fin = np.isfinite(sr) & np.isfinite(si) & (n > 0)
            m64 = s64 / np.maximum(n, 1)
            bound = np.maximum(n - 1, 0) * 2.0 ** -24 * sabs / np.maximum(n, 1) + half_ulp32(m64)
            bad = fin & ~(np.abs(a.astype(np.float64) - m64) <= bound)
        if bad.any():
            out.append("%s: %d channel means outside the summation bound of the float64 mean" % (part, bad.sum()))
    return out


def ref_lowpass(avg, taylor):
    """The first min(taylor, nchan) Fourier bins of each spectrum, by a direct DFT and inverse in long double.
    Returns (re, im) as long double arrays."""
    n_cp, F = avg.shape
    K = min(int(taylor), F)
    kf = (np.arange(K, dtype=np.int64)[:, None] * np.arange(F, dtype=np.int64)[None, :]) % F
    ang = (L(2) * PI_L) * kf.astype(L) / L(F)
    c, s = np.cos(ang), np.sin(ang)                                  # (K, F)
    re, im = avg.real.astype(L), avg.imag.astype(L)
    xr = re @ c.T + im @ s.T                                         # (re + i im) (c - i s)
    xi = im @ c.T - re @ s.T
    return (xr @ c - xi @ s) / L(F), (xr @ s + xi @ c) / L(F)


def lowpass_errors(avg, smooth, taylor):
    n_cp, F = avg.shape
    K = min(int(taylor), F)
    er, ei = ref_lowpass(avg, taylor)
    mean_abs = np.hypot(avg.real.astype(np.float64), avg.imag.astype(np.float64)).mean(axis=1)[:, None]
    f64 = LOWPASS_F64_FACTOR * K * F * 2.0 ** -53 * mean_abs
    out = []
    for part, exact, got in (("re", er, smooth.real), ("im", ei, smooth.imag)):
        bad = ~(np.abs(got.astype(L) - exact) <= (half_ulp32(exact) + f64).astype(L))
        if bad.any():
            out.append("smooth.%s: %d values outside the bound of the long double DFT (first at %s)" % (part, bad.sum(), np.argwhere(bad)[0].tolist()))
        if taylor >= F:                                              # every bin kept: the exact result is avg itself
            a = getattr(avg, "real" if part == "re" else "imag")
            if not (np.abs(exact - a.astype(L)) <= 64 * F * np.finfo(L).eps * mean_abs.astype(L)).all():
                out.append("smooth.%s: the long double DFT does not return avg with every bin kept" % part)
            if not (np.abs(got.astype(np.float64) - a) <= half_ulp32(a) + f64).all():
                out.append("smooth.%s: not avg with every bin kept" % part)
    return out


def ref_resid(oracle, vis, smooth):
    z = np.empty(vis.shape, np.complex64)
    with np.errstate(all="ignore"):
        z.real = vis.real - smooth.real[:, None, :]
        z.imag = vis.imag - smooth.imag[:, None, :]
    return oracle.abs_c64(z)


def ref_medians(absres, mflags):
    """(n_cp, 2): the median of absres[~mflags] and of | |absres| - float32(median) | over the same samples."""
    out = np.full((absres.shape[0], 2), np.nan)
    with np.errstate(all="ignore"):
        for p in range(absres.shape[0]):
            vals = absres[p][mflags[p] == 0]
            if vals.size:
                out[p, 0] = _np_median_abs(vals)
                diff = np.abs(np.abs(vals) - np.float32(out[p, 0]))
                assert diff.dtype == np.float32
                out[p, 1] = _np_median_abs(diff)
    return out


def ref_decide(absres, mad, start, cnt, do_or, sigma=SIGMA):
    n_cp, T, F = absres.shape
    with np.errstate(all="ignore"):
        thr = (np.float32(sigma) * mad.astype(np.float32)).astype(np.float32)
        new = absres > thr[:, None, None]
    out = (start | new) if do_or else new
    out = np.where((cnt == T * F)[:, None, None], start, out)
    return out.astype(np.uint8)


def same_bits(a, b):
    """Equal as bit patterns, or NaN on both sides."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))


def _where(bad):
    return "%d differ, first at %s" % (bad.sum(), np.argwhere(bad)[0].tolist())


def stage_errors(oracle, vis, flags_in, taylor, do_or, tap, out, sigma=SIGMA):
    """Every stage of one cycle, each reference fed with the tapped input of its stage.  `tap`: avg, smooth, absres,
    mflags, med, cnt as host arrays; `out`: the returned flags; `flags_in`: the bytes the cycle started from."""
    n_cp, T, F = vis.shape
    start = flags_in != 0
    rep = []
    cnt = start.reshape(n_cp, -1).sum(axis=1)
    if not np.array_equal(tap["cnt"], cnt):
        rep.append("cnt: %s, expected %s" % (tap["cnt"].tolist(), cnt.tolist()))
    avg = ref_mean(vis, start)[0]
    for part in ("real", "imag"):
        bad = ~same_bits(getattr(tap["avg"], part), getattr(avg, part))
        if bad.any():
            rep.append("avg.%s: %s" % (part, _where(bad)))
    rep += lowpass_errors(tap["avg"], tap["smooth"], taylor)
    absres = ref_resid(oracle, vis, tap["smooth"])
    bad = ~same_bits(tap["absres"], absres)
    if bad.any():
        rep.append("absres: %s" % _where(bad))
    bad = tap["mflags"] != (start | np.isnan(tap["absres"])).astype(np.uint8)
    if bad.any():
        rep.append("mflags: %s" % _where(bad))
    med = ref_medians(tap["absres"], tap["mflags"])
    bad = ~same_bits(tap["med"], med)
    if bad.any():
        rep.append("medians (first, MAD): %s; device %s, expected %s" % (_where(bad), tap["med"].tolist(), med.tolist()))
    exp = ref_decide(tap["absres"], tap["med"][:, 1], start, tap["cnt"], do_or, sigma)
    bad = out != exp
    if bad.any():
        rep.append("flags: %s" % _where(bad))
    if out.max(initial=0) > 1:
        rep.append("flags: bytes other than 0 / 1")
    return rep


def host_cycle(oracle, vis, flags_in, taylor, do_or, sigma=SIGMA):
    """The five references composed into one cycle (the low pass rounded to float32).  Returns (tap, flags)."""
    n_cp, T, F = vis.shape
    start = flags_in != 0
    tap = dict(cnt=start.reshape(n_cp, -1).sum(axis=1).astype(np.uint32), avg=ref_mean(vis, start)[0])
    er, ei = ref_lowpass(tap["avg"], taylor)
    tap["smooth"] = np.empty((n_cp, F), np.complex64)
    tap["smooth"].real, tap["smooth"].imag = er.astype(np.float32), ei.astype(np.float32)
    tap["absres"] = ref_resid(oracle, vis, tap["smooth"])
    tap["mflags"] = (start | np.isnan(tap["absres"])).astype(np.uint8)
    tap["med"] = ref_medians(tap["absres"], tap["mflags"])
    return tap, ref_decide(tap["absres"], tap["med"][:, 1], start, tap["cnt"], do_or, sigma)


def oracle_errors(oracle, vis, flags_in, taylor, do_or, got, sigma=SIGMA):
    """One lock-step cycle of oracle.uvcontsub_flagger from the same flags: every flag of `got` that differs from the
    oracle's must sit within 1e-5 of the oracle's threshold (the criterion of tests/test_uvcontsub.py), and every
    infinite unflagged sample must be flagged."""
    n_cp, T, F = vis.shape
    start = flags_in != 0
    exp, d = oracle.uvcontsub_flagger(vis[:, None], start[:, None], major_cycles=1, or_original_from_cycle=0 if do_or else 1,
                                      taylor_degrees=taylor, sigma=sigma, dump=True)
    exp = exp[:, 0]
    rep = []
    bad = (got != 0) != exp
    if bad.any():
        thr = np.broadcast_to(d["thr"][:, None, None], vis.shape)
        with np.errstate(all="ignore"):
            rel = np.abs(d["absres"] - thr)[bad] / thr[bad]
        if not (rel < 1e-5).all():
            rep.append("oracle: %d flags differ, %d of them not borderline (%s)" % (bad.sum(), (~(rel < 1e-5)).sum(), np.argwhere(bad)[0].tolist()))
    inf = infinite_samples(vis) & ~start & (start.reshape(n_cp, -1).sum(axis=1) < T * F)[:, None, None]
    if inf.any() and not ((got != 0)[inf].all() and exp[inf].all()):
        rep.append("an unflagged infinite sample is not flagged (device or host %s, oracle %s)" % ((got != 0)[inf].tolist(), exp[inf].tolist()))
    return rep


def do_or_of(case, cycle):
    return cycle >= case["or_from"]


# ---------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------
def _placed(a, offset_elements):
    """A contiguous device copy of `a` whose base lies `offset_elements` elements past an aligned (>= 256 B) address."""
    import torch
    t = torch.from_numpy(np.array(a))
    flat = torch.empty(t.numel() + offset_elements, dtype=t.dtype, device="cuda")
    flat[offset_elements:].copy_(t.reshape(-1))
    out = flat[offset_elements:].view(t.shape)
    assert out.data_ptr() % 256 == (offset_elements * t.element_size()) % 256 and out.is_contiguous()
    return out


GUARD = 64


def device_call(vis, flags, taylor, or_from, cycles, sigma=SIGMA, offset=0, ws_products=None, taps=True):
    """tri_uvcontsub_flagger_debug (taps=False: tri_uvcontsub_flagger) through the C ABI.  Returns (rc, flags, tap)."""
    import torch
    from tricolour_amd import _lib
    lib = _lib.lib()
    n_cp, T, F = vis.shape
    N = T * F
    dv = torch.view_as_real(_placed(vis, offset))
    df = _placed(flags, offset)
    raw = torch.full((2 * GUARD + offset + n_cp * N,), 0xA5, dtype=torch.uint8, device="cuda")
    out = raw[GUARD + offset:GUARD + offset + n_cp * N]
    assert (out.data_ptr() - offset) % 64 == 0
    nbytes = lib.tri_uvcontsub_workspace_bytes(ws_products or n_cp, T, F)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    st = torch.cuda.current_stream().cuda_stream
    head = (dv.data_ptr(), df.data_ptr(), out.data_ptr(), n_cp, T, F, int(cycles), int(or_from), int(taylor), float(sigma),
            ws.data_ptr(), nbytes, st)
    tap = None
    if taps:
        # one guarded buffer per tap, filled with a pattern no stage produces
        t = dict(avg=torch.full((n_cp, F, 2), -77.0, dtype=torch.float32, device="cuda"),
                 smooth=torch.full((n_cp, F, 2), -77.0, dtype=torch.float32, device="cuda"),
                 absres=torch.full((n_cp, T, F), -77.0, dtype=torch.float32, device="cuda"),
                 mflags=torch.full((n_cp, T, F), 0xA5, dtype=torch.uint8, device="cuda"),
                 med=torch.full((n_cp, 2), -77.0, dtype=torch.float64, device="cuda"),
                 cnt=torch.full((n_cp,), 0x5A5A5A5, dtype=torch.int32, device="cuda"))
        rc = lib.tri_uvcontsub_flagger_debug(*head, *(t[k].data_ptr() for k in ("avg", "smooth", "absres", "mflags", "med", "cnt")))
        torch.cuda.synchronize()
        tap = {k: v.cpu().numpy() for k, v in t.items()}
        tap["avg"], tap["smooth"] = (np.ascontiguousarray(tap[k]).view(np.complex64)[..., 0] for k in ("avg", "smooth"))
        tap["cnt"] = tap["cnt"].view(np.uint32)
    else:
        rc = lib.tri_uvcontsub_flagger(*head)
        torch.cuda.synchronize()
    host = raw.cpu().numpy()
    lo = GUARD + offset
    assert np.all(host[:lo] == 0xA5) and np.all(host[lo + n_cp * N:] == 0xA5), "bytes outside the output flags were written"
    return rc, host[lo:lo + n_cp * N].reshape(n_cp, T, F).copy(), tap


def taps_differ(a, b):
    return [k for k in a if not np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))]


def run_case(oracle, name):
    """The report of one case: [] when every stage of every cycle equalled its reference."""
    c = CASES[name]
    vis, flags = inputs(name)
    rep = []
    if c["cycles"] == 1:
        rc, out, tap = device_call(vis, flags, c["taylor"], c["or_from"], 1, offset=1 if c["variant"] == "offset" else 0)
        if rc:
            return ["rc %d" % rc]
        rep += stage_errors(oracle, vis, flags, c["taylor"], do_or_of(c, 0), tap, out)
        rep += oracle_errors(oracle, vis, flags, c["taylor"], do_or_of(c, 0), out)
        if c["variant"] == "batched":
            # a workspace that holds two products: batches of 2, 2, 1 -- the same flags and the same taps, product for product
            rc, out2, tap2 = device_call(vis, flags, c["taylor"], c["or_from"], 1, ws_products=2)
            if rc:
                return rep + ["batched: rc %d" % rc]
            if not np.array_equal(out, out2):
                rep.append("batched: flags differ from the whole-batch call: %s" % _where(out != out2))
            if taps_differ(tap, tap2):
                rep.append("batched: taps differ from the whole-batch call: %s" % taps_differ(tap, tap2))
        # the production entry point returns the same flags
        rc, out3, _ = device_call(vis, flags, c["taylor"], c["or_from"], 1, offset=1 if c["variant"] == "offset" else 0, taps=False)
        if rc or not np.array_equal(out, out3):
            rep.append("tri_uvcontsub_flagger: rc %d, flags equal to the debug call's: %s" % (rc, np.array_equal(out, out3)))
        return rep
    # several cycles: each one alone from the flags the references expect of the one before, then all in one call
    cur = flags
    for mi in range(c["cycles"]):
        do_or = do_or_of(c, mi)
        rc, out, tap = device_call(vis, cur, c["taylor"], 0 if do_or else 1, 1)
        if rc:
            return rep + ["cycle %d: rc %d" % (mi, rc)]
        rep += ["cycle %d: %s" % (mi, r) for r in stage_errors(oracle, vis, cur, c["taylor"], do_or, tap, out)]
        rep += ["cycle %d: %s" % (mi, r) for r in oracle_errors(oracle, vis, cur, c["taylor"], do_or, out)]
        _, expected = host_cycle(oracle, vis, cur, c["taylor"], do_or)
        if not np.array_equal(out, expected):
            rep.append("cycle %d: flags differ from the composed references: %s" % (mi, _where(out != expected)))
        cur = expected
    rc, out_all, tap_all = device_call(vis, flags, c["taylor"], c["or_from"], c["cycles"])
    if rc:
        return rep + ["all cycles: rc %d" % rc]
    if not np.array_equal(out_all, cur):
        rep.append("all cycles in one call: flags differ from the cycles fed forward: %s" % _where(out_all != cur))
    if taps_differ(tap, tap_all):
        rep.append("all cycles in one call: the last cycle's taps differ: %s" % taps_differ(tap, tap_all))
    return rep


class Proof:
    def __init__(self):
        self.reports, self.logs, self.met, self.trouble = {}, {}, set(), None


@pytest.fixture(scope="module")
def proof(gpu, oracle):
    """Runs every case once, whatever tests were selected.  After a case that raised (a device fault shows as an
    exception) nothing more is started on the device."""
    import torch
    from tricolour_amd import _lib
    p = Proof()
    for name in CASES:
        if p.trouble:
            p.reports[name] = ["not run: " + p.trouble]
            continue
        _lib.kernel_log_begin()
        try:
            report = run_case(oracle, name)
            torch.cuda.synchronize()
        except Exception:
            report = ["raised:\n" + traceback.format_exc()]
            p.trouble = "the case %s raised" % name
        finally:
            log = _lib.kernel_log_end()
        p.reports[name], p.logs[name] = report, log
        if not report:
            p.met.update(log)
    return p


@gpu_only
@pytest.mark.parametrize("name", list(CASES))
def test_case_matches_the_stage_references(proof, name):
    assert not proof.reports[name], "%s:\n  %s\n  kernels launched: %s" % (
        name, "\n  ".join(proof.reports[name]), sorted(proof.logs.get(name, {})))


_VEC_MED = ["k_medbig_hist<true>", "k_medbig_compact<true>", "k_medbig_select<true>"]
_SCA_MED = ["k_medbig_hist<false>", "k_medbig_compact<false>", "k_medbig_select<false>"]
# which forms each shape is cut for (and, in `absent`, which it must not take), under the default environment
REACH = {
    "3x7x260-K20": (["k_uv_resid4", "k_uv_apply4"] + _VEC_MED, ["k_uv_resid", "k_uv_apply"] + _SCA_MED),
    "2x5x258-K20": (["k_uv_resid", "k_uv_apply"] + _SCA_MED, ["k_uv_resid4", "k_uv_apply4"] + _VEC_MED),
    "2x6x258-K20": (["k_uv_resid", "k_uv_apply4"] + _VEC_MED, ["k_uv_resid4", "k_uv_apply"] + _SCA_MED),
    "3x7x260-K20-offset base": (["k_uv_resid", "k_uv_apply"] + _VEC_MED, ["k_uv_resid4", "k_uv_apply4"] + _SCA_MED),
    "2x33x2050-K0": (["k_uv_resid", "k_uv_apply"] + _SCA_MED, ["k_uv_resid4", "k_uv_apply4"] + _VEC_MED),
    "2x32x2052-K0": (["k_uv_resid4", "k_uv_apply4"] + _VEC_MED, ["k_uv_resid", "k_uv_apply"] + _SCA_MED),
    "2x3x5-K0": (["k_uv_resid", "k_uv_apply"] + _SCA_MED, ["k_uv_resid4", "k_uv_apply4"] + _VEC_MED),
}


def _launched(log, frag):
    # "k_uv_resid" must not count k_uv_resid4: `matches` compares whole base names
    return sum(n for k, n in log.items() if matches(frag, k))


@gpu_only
def test_cases_reach_the_forms_they_were_cut_for(proof):
    import os
    assert not os.environ.get("TRI_UV_SCALAR"), "the scalar kernels must be met under the default environment"
    assert set(REACH) <= set(CASES)
    wrong = []
    for name, (present, absent) in REACH.items():
        log = proof.logs.get(name, {})
        wrong += ["%s does not launch %s: %s" % (name, f, sorted(log)) for f in present if not _launched(log, f)]
        wrong += ["%s launches %s" % (name, f) for f in absent if _launched(log, f)]
    # three batches: the batched call launches the mean three times, the whole-batch calls (debug and production) once each
    for name in ("5x7x260-K20-batches of 2", "5x7x260-K0-batches of 2"):
        n = _launched(proof.logs.get(name, {}), "k_uv_mean")
        if n != 5:
            wrong.append("%s launched k_uv_mean %d times, not 1 + 3 + 1" % (name, n))
    assert not wrong, "\n".join(wrong)


@gpu_only
def test_too_many_taylor_degrees_is_unsupported_without_a_launch(gpu):
    from tricolour_amd import _lib
    vis, flags = inputs("2x3x5-K1")
    _lib.kernel_log_begin()
    try:
        rc, _, _ = device_call(vis, flags, 65, 0, 1)
    finally:
        log = _lib.kernel_log_end()
    assert rc == _lib.TRI_EUNSUPPORTED and not log, (rc, log)
    rc, _, _ = device_call(vis, flags, 65, 0, 1, taps=False)
    assert rc == _lib.TRI_EUNSUPPORTED


@gpu_only
def test_no_cycle_leaves_the_taps_untouched(gpu):
    vis, flags = inputs("2x3x5-K1")
    rc, out, tap = device_call(vis, flags, 20, 0, 0)
    assert rc == 0 and np.array_equal(out, (flags != 0).astype(np.uint8))
    assert (tap["avg"].real == -77).all() and (tap["smooth"].imag == -77).all() and (tap["absres"] == -77).all()
    assert (tap["mflags"] == 0xA5).all() and (tap["med"] == -77).all() and (tap["cnt"] == 0x5A5A5A5).all()


@gpu_only
def test_every_uvcontsub_instantiation_met_its_stage_references(proof):
    """All fourteen instantiations behind tri_uvcontsub_flagger were launched by a case that passed every stage check,
    and nothing else was launched but k_normalise_flags (the fixture has run every case, whatever was selected)."""
    wanted = reachable_instances(UV_CLOSING)
    assert sorted(wanted) == sorted(["k_uv_mean", "k_uv_lowpass", "k_uv_resid", "k_uv_resid4", "k_uv_apply", "k_uv_apply4", "k_medbig_range",
                                     "k_medbig_pick"] + _VEC_MED + _SCA_MED), wanted
    unmet = [frag for frag in wanted if not any(matches(frag, k) for k in proof.met)]
    failed = sorted(n for n, r in proof.reports.items() if r)
    assert not unmet, "no case that passed its stage checks launched %s\nfailed cases: %s" % (unmet, failed)
    every = set().union(*proof.logs.values()) if proof.logs else set()
    stray = sorted(k for k in every if k != "k_normalise_flags" and not any(matches(frag, k) for frag in wanted))
    assert not stray, "kernels launched that are not uvcontsub's: %s" % stray


# ---------------------------------------------------------------------------
# without a device: the references against each other and against the oracle
# ---------------------------------------------------------------------------
def test_the_cases_hold_what_they_were_built_for():
    assert {k for c in CASES.values() for k in c["kinds"]} == KINDS
    # every shape carries every kind it can hold; so does each call variant, and the three-cycle case the kinds whose
    # flags change from cycle to cycle or must not
    for shape in {c["shape"] for c in CASES.values()}:
        held = {k for c in CASES.values() if c["shape"] == shape for k in c["kinds"]}
        assert held == kinds_a_shape_can_hold(shape), (shape, held ^ kinds_a_shape_can_hold(shape))
    for variant in ("offset", "batched"):
        held = {k for c in CASES.values() if c["variant"] == variant for k in c["kinds"]}
        assert held == KINDS - {"overfill"}, (variant, held ^ KINDS)
    for c in CASES.values():
        assert c["taylor"] == 0 or not {"const", "tie", "overfill"} & set(c["kinds"]), c
        assert c["taylor"] < c["shape"][2] or "one" not in c["kinds"], c
    assert {c["taylor"] for c in CASES.values()} == {0, 1, 20, 64}
    assert {c["shape"] for c in CASES.values()} == {(1, 1, 1), (2, 3, 5), (3, 7, 260), (5, 7, 260), (2, 5, 258), (2, 6, 258), (2, 33, 2050), (2, 32, 2052)}
    assert {(c["or_from"], c["cycles"]) for c in CASES.values()} == {(0, 1), (1, 1), (1, 3)}
    for name, c in CASES.items():
        vis, flags = inputs(name)
        n, T, F = c["shape"]
        for p, kind in enumerate(c["kinds"]):
            fl, v = flags[p], vis[p]
            if kind == "general" and T * F >= 6:
                assert {2, 255} <= set(np.unique(fl)) and fl[:, F // 2].all() and (np.isnan(v.real) & (fl == 0)).sum() == 1
            elif kind == "allflag":
                assert fl.all()
            elif kind == "one":
                assert (fl == 0).sum() == 1
            elif kind == "const":
                assert (v == 2 - 1j).all() and (fl == 0).any()
            elif kind == "tie":
                z = np.flatnonzero((v.reshape(-1) == 0) & (fl.reshape(-1) == 0))
                assert z.size == 4 and sorted(z % 4) == [0, 1, 2, 3] and (v.reshape(-1)[np.setdiff1d(np.arange(T * F), z)] == 2 - 1j).all()
            elif kind == "nanonly":
                assert (fl == 0).sum() == min(2, T * F) and (np.isnan(v.real) | np.isnan(v.imag))[fl == 0].all()
            elif kind == "inf1":
                assert (infinite_samples(v) & (fl == 0)).sum() == 1
            elif kind == "infpm":
                f = np.flatnonzero(infinite_samples(v).any(axis=0))
                assert f.size == 1 and sorted(v[:2, f[0]].real) == [-np.inf, np.inf] and not fl[:2, f[0]].any()
            elif kind == "wide":
                a = np.abs(v)
                assert np.log2(a.max() / a.min()) > 29.99


def test_the_overfill_product_overfills_the_centred_candidate_list(oracle):
    """With taylor_degrees = 0 more than 32768 (MEDBIG_CAND) unflagged samples of product 0 share the centred key that
    is the MAD, so no histogram bin around it fits the candidate list: the select must scan the whole window."""
    name = "2x32x2052-K0"
    vis, flags = inputs(name)
    tap, _ = host_cycle(oracle, vis, flags, 0, True)
    assert tap["med"][0].tolist() == [2.0, 1.0]
    keys = np.abs(tap["absres"][0] - np.float32(2.0))
    assert (keys == 1.0).sum() == 40000 > 32768 and (keys < 1.0).sum() == 0
    a = tap["absres"][0]
    assert np.log2(a.max() / a.min()) > 29


@pytest.mark.parametrize("name", list(CASES))
def test_mean_rule_lies_within_the_summation_bound_of_the_float64_mean(name):
    vis, flags = inputs(name)
    assert not mean_bound_errors(vis, flags != 0)


def test_mean_rule_zeroes_what_the_reference_zeroes():
    """np.nanmean followed by avg[isnan(avg)] = 0 (the oracle's restatement of flagging.py:1037-1044) gives 0 for a channel
    with an infinite unflagged sample; so does ref_mean, and the same channels only."""
    for name, channels in (("3x7x260-K20", 2), ("2x5x258-K20", 1)):
        vis, flags = inputs(name)
        start = flags != 0
        avg, n, sr, si = ref_mean(vis, start)
        raw = ref_mean(vis, start, zero_nonfinite=False)[0]
        masked = vis.copy()
        masked[start] = np.nan
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with np.errstate(all="ignore"):
                numpy_avg = np.nanmean(masked, axis=1)
        reset = np.isnan(numpy_avg) & (n > 0)
        infch = (infinite_samples(vis) & ~start).any(axis=1)
        assert infch.sum() == channels and np.array_equal(reset, infch)
        assert (avg[infch] == 0).all() and not np.isfinite(raw[infch].view(np.float32).reshape(-1, 2)).all(axis=1).any()
        assert np.array_equal(avg[~infch], raw[~infch])


def test_half_ulp32():
    assert half_ulp32(1.0) == 2.0 ** -24 and half_ulp32(1.9999) == 2.0 ** -24 and half_ulp32(2.0) == 2.0 ** -23
    assert half_ulp32(0.0) == 2.0 ** -150 and half_ulp32(-3.0) == 2.0 ** -23


def test_long_double_lowpass_agrees_with_the_fft():
    rs = np.random.RandomState(5)
    avg = (rs.standard_normal((2, 37)) + 1j * rs.standard_normal((2, 37))).astype(np.complex64)
    for K in (0, 1, 20, 64):
        spec = np.fft.fft(avg.astype(np.complex128), axis=1)
        spec[:, K:] = 0
        exp = np.fft.ifft(spec, axis=1)
        er, ei = ref_lowpass(avg, K)
        assert np.abs(er.astype(np.float64) - exp.real).max() < 1e-13 and np.abs(ei.astype(np.float64) - exp.imag).max() < 1e-13
    assert np.finfo(L).eps <= 2.0 ** -52


@pytest.mark.parametrize("name", list(CASES))
def test_composed_references_against_the_oracle(oracle, name):
    """The five references composed into whole cycles pass their own stage checks (so the checks need no device to be
    exercised) and, lock-step from the same flags, differ from oracle.uvcontsub_flagger in borderline flags only; the
    infinite samples are flagged by both."""
    c = CASES[name]
    vis, cur = inputs(name)
    for mi in range(c["cycles"]):
        do_or = do_or_of(c, mi)
        tap, out = host_cycle(oracle, vis, cur, c["taylor"], do_or)
        assert not stage_errors(oracle, vis, cur, c["taylor"], do_or, tap, out)
        assert not oracle_errors(oracle, vis, cur, c["taylor"], do_or, out)
        start = cur != 0
        full = start.reshape(start.shape[0], -1).all(axis=1)
        assert np.array_equal(out[full], start[full].astype(np.uint8))
        for p, kind in enumerate(c["kinds"]):
            if kind == "tie":                                    # residuals exactly on the threshold stay unflagged
                on = (tap["absres"][p] == 0) & ~start[p]
                assert tap["med"][p, 1] == 0 and on.sum() == 4 and not out[p][on].any() and out[p][~on].all()
        cur = out


def test_stage_checks_notice_a_wrong_stage(oracle):
    """Each stage check fails when its stage alone is off by the least amount."""
    name = "3x7x260-K20"
    c = CASES[name]
    vis, flags = inputs(name)
    tap, out = host_cycle(oracle, vis, flags, c["taylor"], True)

    def errs(**changed):
        t = dict(tap, **{k: v for k, v in changed.items() if k != "out"})
        return " ".join(stage_errors(oracle, vis, flags, c["taylor"], True, t, changed.get("out", out)))
    up = lambda a: np.nextafter(a, np.float32(np.inf))
    a = tap["avg"].copy(); a.real[0, 259] = up(a.real[0, 259])
    assert "avg.real" in errs(avg=a)
    s = tap["smooth"].copy(); s.imag[2, 3] = up(up(s.imag[2, 3]))
    assert "smooth.im" in errs(smooth=s)
    r = tap["absres"].copy(); r[0, 6, 258] = up(r[0, 6, 258])
    assert "absres" in errs(absres=r)
    m = tap["mflags"].copy(); m[0, 0, 0] ^= 1
    assert "mflags" in errs(mflags=m)
    d = tap["med"].copy(); d[0, 1] = np.nextafter(np.float32(d[0, 1]), np.float32(0))
    assert "medians" in errs(med=d)
    n = tap["cnt"].copy(); n[1] += 1
    assert "cnt" in errs(cnt=n)
    o = out.copy(); o[0, 3, 3] ^= 1
    assert "flags" in errs(out=o)
