"""Piecewise-polynomial fit flagging (``polyfit_background``, ``threshold_polyfit``, after CASA's tfcrop): the NumPy
restatement of the definition (``include/tricolour_amd.h``) against a literal per-sample loop in Python floats, the
contents that reach each branch of the definition, the behaviour on noise with injected interference, the argument
checks and the ABI on the CPU; the device kernels against the restatement on the GPU.

No tolerance anywhere.  Every operation of the definition is a single correctly rounded float64 operation in a fixed
order -- the moments and the residual power as two-level sums over cells of 32 samples, the Cholesky factor, the
substitutions and Horner's rule term by term -- so the hits must agree exactly and the background in every bit (every
NaN of the definition is 0x7FC00000, in the restatement and on the device alike).

This module also keeps the kernel table of ``tricolour_amd/csrc/steps/polyfit/``: KERNELS lists every ``__global__``
kernel there with each instantiation a launch site can produce; a CPU test holds it to the sources, and the last GPU
test shows with the library's kernel log that every listed instantiation was launched by a call whose result was
compared with the restatement."""
import contextlib
import ctypes as C
import glob
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_median_zscore import NAN32, amplitude, dev, differing, same_bits
import test_median_zscore as tmz

CELL = 32               # PF_CELL of kernels_polyfit.hpp: samples per cell of the two-level sums
MAX_PIECES = 32         # PF_MAX_PIECES
MAX_LINE = 16384        # PF_MAX_LINE: longest fitted line
MAX_ROUNDS = 16         # PF_MAX_ROUNDS
SMALL_LINE = 4096       # the frequency pass keeps lines up to this length in its smaller LDS arrays
GUARD = 2.0 ** -20
ORDERS = ("freqtime", "timefreq", "freq", "time")
DEFAULTS = dict(time_cutoff=4.0, time_degree=1, time_pieces=1, freq_cutoff=3.0, freq_degree=3, freq_pieces=7, rounds=5,
                min_samples=8)

# every __global__ kernel of csrc/steps/polyfit/ and its instantiations, in the spelling of the kernel log
# (k_pf_prepare<VIS, VEC>: VIS 0 = complex64, 1 = float32, VEC: 4 samples per lane; k_pf_freq<CAP, BG>: CAP the line
# capacity of the LDS arrays, BG the background call; k_pf_time<BG>; k_pf_finish<VEC>: 16 samples per lane)
KERNELS = {"k_pf_prepare": {"k_pf_prepare<0, false>", "k_pf_prepare<0, true>", "k_pf_prepare<1, false>",
                            "k_pf_prepare<1, true>"},
           "k_pf_freq": {"k_pf_freq<4096, false>", "k_pf_freq<4096, true>", "k_pf_freq<16384, false>",
                         "k_pf_freq<16384, true>"},
           "k_pf_time": {"k_pf_time<false>", "k_pf_time<true>"},
           "k_pf_finish": {"k_pf_finish<false>", "k_pf_finish<true>"}}
MET = set()        # instantiations launched by calls whose results equalled the restatement


# ---------------------------------------------------------------------------
# the definition, restated: vectorised over lines (and pieces and cells), explicit in sample order
# ---------------------------------------------------------------------------
_LAYOUTS = {}


def layout(n, P):
    """Of a line of n samples in P pieces: idx (P, cells, CELL) the sample of every cell slot (-1: none), x of the same
    shape, and per sample its piece and its x."""
    if (n, P) not in _LAYOUTS:
        e = [(p * n) // P for p in range(P + 1)]
        cells = max(1, max(-(-(e[p + 1] - e[p]) // CELL) for p in range(P)))
        idx = np.full((P, cells * CELL), -1, np.int64)
        x = np.zeros((P, cells * CELL), np.float64)
        piece_of, x_of = np.zeros(n, np.int64), np.zeros(n, np.float64)
        for p in range(P):
            L = e[p + 1] - e[p]
            j = np.arange(L)
            xs = (2 * j + 1 - L).astype(np.float64) / np.float64(L) if L else np.zeros(0)
            idx[p, :L], x[p, :L] = e[p] + j, xs
            piece_of[e[p]:e[p + 1]], x_of[e[p]:e[p + 1]] = p, xs
        out = (idx.reshape(P, cells, CELL), x.reshape(P, cells, CELL), piece_of, x_of)
        for a in out:
            a.setflags(write=False)
        _LAYOUTS[(n, P)] = out
    return _LAYOUTS[(n, P)]


def two_level(values, m, idx):
    """Sum of values (lines, n) float64 over the masked samples of every piece: a sequential chain inside each cell,
    then the cell sums in ascending cell order.  Returns (lines, P)."""
    ok = idx >= 0
    safe = np.where(ok, idx, 0)
    v, mm = values[:, safe], m[:, safe] & ok                       # (lines, P, cells, CELL)
    cell = np.zeros(v.shape[:-1], np.float64)
    for jj in range(CELL):
        cell = np.where(mm[..., jj], cell + v[..., jj], cell)
    total = np.zeros(cell.shape[:-1], np.float64)
    for c in range(cell.shape[-1]):
        total = total + cell[..., c]
    return total


def solve(S, B, n_p, D):
    """The fit of every (line, piece) from its moments S (7, ...) and B (4, ...): c (4, ...) and the degree used (-1: the
    piece holds no sample)."""
    d = np.minimum(D, n_p - 1)
    zero = np.zeros(n_p.shape, np.float64)
    l = [[zero.copy() for _ in range(4)] for _ in range(4)]
    least = GUARD * S[0]
    with np.errstate(all="ignore"):
        for j in range(4):
            act = j <= d
            v = S[2 * j]
            for k in range(j):
                v = v - l[j][k] * l[j][k]
            bad = act & ~(v > least)
            d = np.where(bad, j - 1, d)
            good = act & ~bad
            ljj = np.sqrt(np.where(good, v, 1.0))
            l[j][j] = np.where(good, ljj, 0.0)
            for i in range(j + 1, 4):
                t = S[i + j]
                for k in range(j):
                    t = t - l[i][k] * l[j][k]
                l[i][j] = np.where(good, t / ljj, 0.0)
        y = [zero.copy() for _ in range(4)]
        for i in range(4):
            act = i <= d
            t = B[i]
            for k in range(i):
                t = t - l[i][k] * y[k]
            y[i] = np.where(act, t / np.where(act, l[i][i], 1.0), 0.0)
        c = [zero.copy() for _ in range(4)]
        for i in range(3, -1, -1):
            act = i <= d
            t = y[i]
            for k in range(i + 1, 4):
                t = np.where(k <= d, t - l[k][i] * c[k], t)
            c[i] = np.where(act, t / np.where(act, l[i][i], 1.0), 0.0)
    return np.stack(c), d


def fit(A, m, P, D):
    """The fit of lines A (lines, n) float32 under the mask m: f (lines, n) float64, NaN where a piece holds no masked
    sample, and the degree used per (line, piece)."""
    n = A.shape[1]
    idx, x, piece_of, x_of = layout(n, P)
    a64 = A.astype(np.float64)
    with np.errstate(all="ignore"):
        pw = np.ones(n)
        S, B = [], []
        for k in range(7):
            S.append(two_level(np.broadcast_to(pw, a64.shape), m, idx))
            if k < 4:
                B.append(two_level(pw * a64, m, idx))
            pw = pw * x_of
        n_p = (m[:, np.where(idx >= 0, idx, 0)] & (idx >= 0)).sum(axis=(-1, -2))
        c, d = solve(np.stack(S), np.stack(B), n_p, D)
        cs, dd = c[:, :, piece_of], d[:, piece_of]
        f = cs[3]
        f = np.where(dd == 2, cs[2], np.where(dd > 2, f * x_of + cs[2], f))
        f = np.where(dd == 1, cs[1], np.where(dd > 1, f * x_of + cs[1], f))
        f = np.where(dd == 0, cs[0], f * x_of + cs[0])
        f = np.where(dd < 0, np.nan, f)
    return f, d


def schedule(r, max_pieces, degree):
    return min(2 * r + 1, max_pieces), (min(1, degree) if r == 0 else degree)


def robust_rounds(A, m0, max_pieces, degree, cutoff, rounds, min_samples, trace=None):
    """The hits (lines, n) of the rounds on lines A under the starting mask m0."""
    hit = np.zeros(m0.shape, bool)
    alive = np.ones(len(A), bool)
    a64 = A.astype(np.float64)
    for r in range(rounds):
        m = m0 & ~hit
        P, D = schedule(r, max_pieces, degree)
        n_m = m.sum(axis=1)
        alive &= n_m >= min_samples
        if not alive.any():
            break
        f, d = fit(A, m, P, D)
        with np.errstate(all="ignore"):
            res = a64 - f
            idx = layout(A.shape[1], P)[0]
            Q = np.zeros(len(A))
            per_piece_cells = two_level_cells(res * res, m, idx)
            for p in range(per_piece_cells.shape[1]):
                for c in range(per_piece_cells.shape[2]):
                    Q = Q + per_piece_cells[:, p, c]
            limit = cutoff * np.sqrt(Q / n_m.astype(np.float64))
            over = np.abs(res) > limit[:, None]
            new = m & over & (np.abs(res) > np.abs(f) * GUARD) & alive[:, None]
        if trace is not None:
            trace.append(dict(m=m, f=f, res=res, limit=limit, over=m & over & alive[:, None], new=new, d=d, P=P, D=D))
        hit |= new
    return hit


def two_level_cells(values, m, idx):
    """The cell sums of two_level: (lines, P, cells)."""
    ok = idx >= 0
    safe = np.where(ok, idx, 0)
    v, mm = values[:, safe], m[:, safe] & ok
    cell = np.zeros(v.shape[:-1], np.float64)
    for jj in range(CELL):
        cell = np.where(mm[..., jj], cell + v[..., jj], cell)
    return cell


def lines_of(img, axis):
    """(lines, n) of an image (..., time, chan): the rows for axis "freq", the channels for "time"."""
    if axis == "time":
        img = np.swapaxes(img, -1, -2)
    return np.ascontiguousarray(img).reshape(-1, img.shape[-1])


def image_of(lines, shape, axis):
    if axis == "time":
        return np.swapaxes(lines.reshape(shape[:-2] + (shape[-1], shape[-2])), -1, -2)
    return lines.reshape(shape)


def valid_of(vis, flags):
    a = amplitude(vis)
    return a, (np.asarray(flags) == 0) & np.isfinite(a)


def one_pass(a, m0, axis, kw):
    hit = robust_rounds(lines_of(a, axis), lines_of(m0, axis), kw[axis + "_pieces"], kw[axis + "_degree"],
                        kw[axis + "_cutoff"], kw["rounds"], kw["min_samples"])
    return image_of(hit, a.shape, axis)


def restate(vis, flags, **kw):
    """{order: out (bool)} of the step for all four orders; the first passes are shared."""
    kw = dict(DEFAULTS, **kw)
    a, valid = valid_of(vis, flags)
    flagged = np.asarray(flags) != 0
    hf, ht = one_pass(a, valid, "freq", kw), one_pass(a, valid, "time", kw)
    return {"freq": flagged | hf, "time": flagged | ht,
            "freqtime": flagged | hf | one_pass(a, valid & ~hf, "time", kw),
            "timefreq": flagged | ht | one_pass(a, valid & ~ht, "freq", kw)}


def restate_background(vis, flags, axis, pieces, degree):
    a, valid = valid_of(vis, flags)
    f, _ = fit(lines_of(a, axis), lines_of(valid, axis), pieces, degree)
    with np.errstate(all="ignore"):
        return tmz.canonical(image_of(f.astype(np.float32), a.shape, axis))


# ---- the definition, literally: one line, one sample at a time, in Python floats ----
def loop_fit(a, m, P, D):
    """f (list of float, NaN where the piece holds nothing) and the degree used per piece."""
    n = len(a)
    f, used = [math.nan] * n, []
    for p in range(P):
        e0, e1 = (p * n) // P, ((p + 1) * n) // P
        L = e1 - e0
        S, B, n_p = [0.0] * 7, [0.0] * 4, 0
        for j0 in range(0, L, CELL):
            s, b = [0.0] * 7, [0.0] * 4
            for j in range(j0, min(j0 + CELL, L)):
                if m[e0 + j]:
                    x = float(2 * j + 1 - L) / float(L)
                    pw = 1.0
                    for k in range(2 * D + 1):
                        s[k] += pw
                        if k <= D:
                            b[k] += pw * float(a[e0 + j])
                        pw = pw * x
                    n_p += 1
            S = [S[k] + s[k] for k in range(7)]
            B = [B[k] + b[k] for k in range(4)]
        if n_p == 0:
            used.append(-1)
            continue
        d = min(D, n_p - 1)
        l = [[0.0] * 4 for _ in range(4)]
        j = 0
        while j <= d:
            v = S[2 * j]
            for k in range(j):
                v = v - l[j][k] * l[j][k]
            if not v > GUARD * S[0]:
                d = j - 1
                break
            l[j][j] = math.sqrt(v)
            for i in range(j + 1, d + 1):
                t = S[i + j]
                for k in range(j):
                    t = t - l[i][k] * l[j][k]
                l[i][j] = t / l[j][j]
            j += 1
        y, c = [0.0] * 4, [0.0] * 4
        for i in range(d + 1):
            t = B[i]
            for k in range(i):
                t = t - l[i][k] * y[k]
            y[i] = t / l[i][i]
        for i in range(d, -1, -1):
            t = y[i]
            for k in range(i + 1, d + 1):
                t = t - l[k][i] * c[k]
            c[i] = t / l[i][i]
        for j in range(L):
            x = float(2 * j + 1 - L) / float(L)
            v = c[d]
            for k in range(d - 1, -1, -1):
                v = v * x + c[k]
            f[e0 + j] = v
        used.append(d)
    return f, used


def loop_rounds(a, m0, max_pieces, degree, cutoff, rounds, min_samples):
    n = len(a)
    hit = [False] * n
    for r in range(rounds):
        m = [bool(m0[i]) and not hit[i] for i in range(n)]
        P, D = schedule(r, max_pieces, degree)
        n_m = sum(m)
        if n_m < min_samples:
            break
        f, _ = loop_fit(a, m, P, D)
        Q = 0.0
        for p in range(P):
            e0, e1 = (p * n) // P, ((p + 1) * n) // P
            for j0 in range(0, e1 - e0, CELL):
                q = 0.0
                for i in range(e0 + j0, min(e0 + j0 + CELL, e1)):
                    if m[i]:
                        res = float(a[i]) - f[i]
                        q = q + res * res
                Q = Q + q
        sigma = math.sqrt(Q / float(n_m))
        for i in range(n):
            if m[i]:
                res = float(a[i]) - f[i]
                if abs(res) > cutoff * sigma and abs(res) > abs(f[i]) * GUARD:
                    hit[i] = True
    return hit


def same_f64(a, b):
    """The same bits, any NaN equal to any NaN."""
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def truncated_at(d, n_p, D):
    """The Cholesky column at which the degree truncation fired per (line, piece), 0 where it did not."""
    return np.where((n_p > 0) & (d < np.minimum(D, n_p - 1)), d + 1, 0)


def pairwise(a):
    """Tree sum over axis 0."""
    return a[0] if len(a) == 1 else pairwise(a[:len(a) // 2]) + pairwise(a[len(a) // 2:])


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
CONTENTS = ["noise", "flags30", "truncate", "few", "all_flagged", "nonfinite", "huge", "tiny", "constant", "ramp"]


def make_case(shape, seed, dtype="c64", content="noise"):
    """(vis, flags): `content` names what the windows hold -- Rayleigh noise on a slowly varying level with 3 % spikes
    and, beyond that,
      truncate   all but 2, 3 or 4 adjacent channels of every row flagged: the usable ones cluster in a corner of a piece
      few        per line, by turns: no usable sample, one, D, and one fewer than min_samples = 8
      huge/tiny  amplitudes near 1e30 / 1e-30
      constant   one value everywhere
      ramp       an exact float32 ramp near 1e6: what is left over a line fit is rounding residue"""
    rng = np.random.default_rng(seed + 2000)
    vis = tmz.make_vis(shape, seed, dtype)
    flags = np.zeros(shape, bool)
    spikes = rng.uniform(size=shape) < 0.03
    vis[spikes] *= np.float32(20)
    T, F = shape[-2:]
    if content == "flags30":
        flags = rng.uniform(size=shape) < 0.3
    elif content == "truncate":
        flags[:] = True
        for t in range(T):
            k = 2 + t % 3                                               # 2, 3, 4 adjacent channels
            c0 = (7 * t + F // 3) % max(1, F - k)
            flags[..., t, c0:c0 + k] = False
    elif content == "few":
        flags[:] = True
        for t in range(T):
            flags[..., t, : (0, 1, 3, 7)[t % 4]] = False
    elif content == "all_flagged":
        flags[:] = True
    elif content == "nonfinite":
        vis, flags = tmz.make_case(shape, seed, dtype, "nonfinite")
    elif content == "huge":
        vis = (vis * np.float32(1e30)).astype(vis.dtype)
    elif content == "tiny":
        vis = (vis * np.float32(1e-30)).astype(vis.dtype)
    elif content == "constant":
        vis[:] = vis.reshape(-1)[0]
    elif content == "ramp":
        ramp = (np.float32(1e6) + np.float32(0.37) * np.arange(F, dtype=np.float32)
                + np.float32(0.11) * np.arange(T, dtype=np.float32)[:, None]).astype(np.float32)
        vis = np.broadcast_to(ramp, shape).astype(vis.dtype)
    else:
        assert content == "noise"
    return vis, flags


def behaviour_input(seed=4):
    """48 x 200 Rayleigh amplitudes on a curved bandpass with one channel raised, one row raised and a 10-sample blob.
    Returns (vis float32, channel mask, row mask, blob mask)."""
    rs = np.random.RandomState(seed)
    T, F = 48, 200
    x = np.linspace(-1, 1, F)
    bandpass = 10.0 * (1.0 - 0.6 * x * x + 0.2 * x)
    vis = bandpass + rs.rayleigh(1.0, (T, F))
    chan, row, blob = (np.zeros((T, F), bool) for _ in range(3))
    chan[:, 60] = True
    row[20, :] = True
    blob[33:35, 140:145] = True
    vis[chan] += 8.0
    vis[row] += 5.0
    vis[blob] += 10.0
    return vis.astype(np.float32), chan, row & ~chan, blob


# ---------------------------------------------------------------------------
# CPU: the restatement, the contents, the behaviour, the argument checks, the ABI, the kernel table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["c64", "f32"])
def test_restatement_equals_the_literal_loop(dtype):
    cases = 0
    for n, content in ((1, "noise"), (7, "flags30"), (33, "noise"), (70, "flags30"), (97, "truncate"), (70, "few"),
                       (40, "nonfinite"), (65, "huge"), (65, "tiny"), (40, "constant"), (64, "ramp"), (12, "all_flagged")):
        vis, flags = make_case((1, 1, 3, n), 11 + n, dtype, content)
        a, valid = valid_of(vis[0, 0], flags[0, 0])
        for pieces, degree, cutoff, rounds, ms in ((1, 0, 3.0, 1, 2), (3, 1, 2.5, 3, 4), (7, 3, 3.0, 5, 8), (32, 2, 2.0, 4, 2)):
            got = robust_rounds(a, valid, pieces, degree, cutoff, rounds, ms)
            for line in range(len(a)):
                want = loop_rounds(list(a[line]), list(valid[line]), pieces, degree, cutoff, rounds, ms)
                assert np.array_equal(got[line], want), (n, content, pieces, degree, line)
                f, d = fit(a[line:line + 1], valid[line:line + 1], pieces, degree)
                lf, ld = loop_fit(list(a[line]), list(valid[line]), pieces, degree)
                assert same_f64(f[0], np.array(lf, np.float64)), (n, content, pieces, degree, line)
                assert list(d[0]) == ld
                cases += 1
    assert cases > 100


def test_the_order_of_the_sums_is_part_of_the_definition():
    """One input on which a pairwise sum of the moments is not the two-level one, down to the bits of the fit."""
    vis, flags = make_case((1, 1, 1, 640), 3, "f32", "noise")
    a, valid = valid_of(vis[0, 0], flags[0, 0])
    f, d = fit(a, valid, 1, 3)
    assert d[0, 0] == 3
    x = layout(640, 1)[3]
    a64 = a[0].astype(np.float64)
    S = np.stack([pairwise(x ** 0 * np.ones(640))] + [pairwise(np.prod([x] * k, axis=0)) for k in range(1, 7)])
    B = np.stack([pairwise(a64)] + [pairwise(np.prod([x] * k, axis=0) * a64) for k in range(1, 4)])
    c, d2 = solve(S[:, None], B[:, None], np.array([640]), 3)
    g = ((c[3, 0] * x + c[2, 0]) * x + c[1, 0]) * x + c[0, 0]
    assert d2[0] == 3 and np.allclose(g, f[0], rtol=1e-9)
    assert (g != f[0]).any()                       # otherwise the case proves nothing


def test_contents_reach_what_they_are_for():
    # degree truncation at j = 1: two adjacent usable samples in a 2100-channel single piece give the mean
    a = np.linspace(1, 2, 2100, dtype=np.float32)[None]
    m = np.zeros((1, 2100), bool)
    m[0, 1000:1002] = True
    f, d = fit(a, m, 1, 3)
    mean = (np.float64(a[0, 1000]) + np.float64(a[0, 1001])) / 2.0
    assert d[0, 0] == 0 and np.ptp(f[0]) == 0 and abs(f[0, 0] - mean) <= 4 * np.spacing(mean)
    # the "truncate" content, rows of 2, 3 and 4 adjacent usable channels: j = 1 and j = 2 fire in a 2100-channel piece,
    # j = 3 in a 40-channel one, along either axis
    fired = set()
    for nchan in (2100, 40):
        vis, flags = make_case((1, 1, 6, nchan), 1, "f32", "truncate")
        av, valid = valid_of(vis[0, 0], flags[0, 0])
        assert sorted(set(valid.sum(axis=1))) == [2, 3, 4]
        _, d = fit(av, valid, 1, 3)
        fired |= set(truncated_at(d, valid.sum(axis=1)[:, None], 3).reshape(-1))
    assert fired == {0, 1, 2, 3}, fired
    # n_p <= D: fewer samples than coefficients lowers the degree to n_p - 1; no sample: NaN
    vis, flags = make_case((1, 1, 8, 40), 2, "f32", "few")
    av, valid = valid_of(vis[0, 0], flags[0, 0])
    f, d = fit(av, valid, 1, 3)
    assert list(d[:3, 0]) == [-1, 0, 2] and np.isnan(f[0]).all() and not np.isnan(f[1:4]).any()
    # empty pieces (n < P) hold nothing, the others still fit
    f, d = fit(av[:, :5], np.ones((8, 5), bool), 7, 3)
    assert (np.diff([(p * 5) // 7 for p in range(8)]) == 0).sum() == 2 and not np.isnan(f).any() and (d == -1).sum() == 16
    # a line below min_samples is left alone; the "few" lines never reach 8
    assert not robust_rounds(av, valid, 1, 1, 0.5, 5, 8).any()
    assert robust_rounds(av, valid, 1, 1, 0.5, 5, 2)[2:].any()
    # all flagged, non-finite: no hits there, the others carry on
    vis, flags = make_case((1, 1, 4, 64), 3, "c64", "nonfinite")
    av, valid = valid_of(vis[0, 0], flags[0, 0])
    assert not np.isfinite(av).all() and (~valid).sum() >= 9
    hit = robust_rounds(av, valid, 3, 2, 2.0, 3, 8)
    assert hit.any() and not hit[~valid].any()
    assert restate(*make_case((1, 1, 9, 40), 4, "c64", "all_flagged"))["freqtime"].all()
    # 1e30 and 1e-30: every moment, factor and residual stays finite and regular, and the rounds still hit the spikes
    for content in ("huge", "tiny"):
        vis, flags = make_case((1, 1, 12, 90), 5, "f32", content)
        av, valid = valid_of(vis[0, 0], flags[0, 0])
        assert (av.max() > 1e30) if content == "huge" else (0 < av.max() < 1e-28)
        hit = robust_rounds(av, valid, 3, 3, 3.0, 5, 8)
        assert 0 < hit.sum() < hit.size // 4
    # a constant image: no hits, whatever the cutoff
    vis, flags = make_case((1, 1, 12, 90), 6, "c64", "constant")
    for out in restate(vis, flags, time_cutoff=0.5, freq_cutoff=0.5).values():
        assert not out.any()
    # the guard decides: the ramp's residue over a line fit passes cutoff * sigma and not |f| 2^-20
    vis, flags = make_case((1, 1, 6, 200), 7, "f32", "ramp")
    av, valid = valid_of(vis[0, 0], flags[0, 0])
    trace = []
    hit = robust_rounds(av, valid, 1, 1, 1.0, 2, 8, trace)
    assert not hit.any() and trace[0]["over"].sum() > 100 and (trace[0]["limit"] > 0).all()


def test_behaviour_channel_row_and_blob_are_hit_and_noise_is_not():
    """Measured with this restatement (RandomState(4), the defaults, order freqtime): the raised channel hit 100 %, the
    raised row 99.5 %, the blob 100 %, clean samples 0.83 %; pure Rayleigh noise (RandomState(5)) 0.74 %.  The asserted
    bounds are conditions with margin, not the figures."""
    vis, chan, row, blob = behaviour_input()
    out = restate(vis[None, None], np.zeros((1, 1) + vis.shape, bool))["freqtime"][0, 0]
    clean = ~(chan | row | blob)
    figures = (out[chan].mean(), out[row].mean(), out[blob].mean(), out[clean].mean())
    print("channel %.3f row %.3f blob %.3f clean %.4f" % figures)
    assert out[chan].all() and out[blob].all()
    assert figures[1] >= 0.85
    assert figures[3] <= 0.03
    rs = np.random.RandomState(5)
    noise = rs.rayleigh(1.0, (1, 1, 48, 200)).astype(np.float32)
    frac = restate(noise, np.zeros(noise.shape, bool))["freqtime"].mean()
    print("pure noise %.4f" % frac)
    assert frac <= 0.03


def test_python_argument_errors_come_before_any_device_work():
    from tricolour_amd import flagging
    vis = np.zeros((3, 1, 4, 8), np.complex64)
    flags = np.zeros((3, 1, 4, 8), bool)
    for fn in (flagging.polyfit_background, flagging.threshold_polyfit):
        with pytest.raises(ValueError):
            fn(vis, flags[:, :, :3])                               # a shape mismatch
        with pytest.raises(ValueError):
            fn(vis[0], flags[0])                                   # not 4-D
        for bad in (np.zeros(vis.shape, np.float64), np.zeros(vis.shape, np.complex128), np.zeros(vis.shape, np.int32)):
            with pytest.raises(ValueError, match="complex64 or float32"):
                fn(bad, flags)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(order="both"), dict(order=None), dict(order=0), dict(time_cutoff=0), dict(time_cutoff=-1.0),
               dict(time_cutoff=nan), dict(time_cutoff=inf), dict(time_cutoff="x"), dict(time_cutoff=True),
               dict(freq_cutoff=0.0), dict(freq_cutoff=nan), dict(freq_cutoff=None), dict(time_degree=-1),
               dict(time_degree=4), dict(time_degree=1.5), dict(time_degree=True), dict(freq_degree=4),
               dict(freq_degree="3"), dict(time_pieces=0), dict(time_pieces=33), dict(freq_pieces=0),
               dict(freq_pieces=MAX_PIECES + 1), dict(freq_pieces=2.5), dict(rounds=0), dict(rounds=MAX_ROUNDS + 1),
               dict(rounds=nan), dict(min_samples=1), dict(min_samples=0), dict(min_samples=2.5), dict(min_samples=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            flagging.threshold_polyfit(vis, flags, **kw)
        with pytest.raises(ValueError, match=next(iter(kw))):
            flagging.check_polyfit_kwargs(**kw)
    for kw in (dict(axis="both"), dict(axis=0), dict(pieces=0), dict(pieces=33), dict(pieces=1.5), dict(degree=-1),
               dict(degree=4), dict(degree=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            flagging.polyfit_background(vis, flags, **kw)
    # the line-length limit comes from the shape alone, before the inputs go anywhere
    for shape, order, axis in (((1, 1, 1, MAX_LINE + 1), "freq", "freq"), ((1, 1, MAX_LINE + 1, 1), "time", "time")):
        long_vis, long_flags = np.zeros(shape, np.float32), np.zeros(shape, bool)
        with pytest.raises(NotImplementedError, match="at most"):
            flagging.threshold_polyfit(long_vis, long_flags, order=order)
        with pytest.raises(NotImplementedError, match="at most"):
            flagging.polyfit_background(long_vis, long_flags, axis)
    assert flagging.check_polyfit_kwargs() == ("freqtime", 4.0, 1, 1, 3.0, 3, 7, 5, 8)
    assert flagging.check_polyfit_kwargs("time", 2, 0, 32, 1, 3, 1, 16, 2) == ("time", 2.0, 0, 32, 1.0, 3, 1, 16, 2)
    assert flagging.PF_ORDERS == ORDERS


def test_header_declares_and_the_binding_exports_the_entry_points():
    from tricolour_amd import _lib
    with open(os.path.join(ROOT, "include", "tricolour_amd.h")) as fh:
        hdr = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in ("tri_polyfit_background", "tri_polyfit_threshold"):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl, name
        assert "stream" in decl.group(1) and "scratch_bytes" in decl.group(1), name
    assert re.search(r"\bsize_t\s+tri_polyfit_workspace_bytes\s*\(", hdr)
    for name in ("tri_polyfit_workspace_bytes", "tri_polyfit_background", "tri_polyfit_threshold"):
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().tri_version() >= 112
    for name in ("kernels_polyfit.hpp", "polyfit_host.hpp"):
        assert os.path.join(ROOT, "tricolour_amd", "csrc", "steps", "polyfit", name) in _lib.DEPENDS


def test_abi_rejects_bad_arguments_without_a_launch():
    from tricolour_amd import _lib
    lib = _lib.lib()
    buf = (C.c_uint8 * ((1 << 20) + 256))()
    base = (C.addressof(buf) + 255) & ~255
    v, f, o, g, ws = base, base + (1 << 18), base + (2 << 18), base + (3 << 18), base + (3 << 18) + (1 << 17)
    nan, inf = float("nan"), float("inf")
    # 2 windows of 4 x 8: vis 512 bytes, flags and out 64, background 256
    need = lib.tri_polyfit_workspace_bytes(2, 4, 8, 1)
    assert need == 256 + 256 + 2 * 5 * 8 * 8 + (-(2 * 5 * 8 * 8) % 256)
    assert lib.tri_polyfit_workspace_bytes(2, 4, 8, 0) == 512
    assert lib.tri_polyfit_workspace_bytes(0, 4, 8, 1) == 0 and lib.tri_polyfit_workspace_bytes(2, 4, 8, 33) == 0
    assert lib.tri_polyfit_workspace_bytes(2, 4, 8, -1) == 0

    def th(vis=v, dtype=_lib.TRI_VIS_C64, flags=f, out=o, n_win=2, ntime=4, nchan=8, order=0, ct=4.0, dt=1, pt=1, cf=3.0,
           df=3, pf=7, rounds=5, ms=8, work=ws, nbytes=need):
        return lib.tri_polyfit_threshold(vis, dtype, flags, out, n_win, ntime, nchan, order, ct, dt, pt, cf, df, pf, rounds,
                                         ms, work, nbytes, None)

    def bg(vis=v, dtype=_lib.TRI_VIS_C64, flags=f, out=g, n_win=2, ntime=4, nchan=8, axis=0, pieces=1, degree=3, work=ws,
           nbytes=need):
        return lib.tri_polyfit_background(vis, dtype, flags, n_win, ntime, nchan, axis, pieces, degree, out, work, nbytes,
                                          None)
    _lib.kernel_log_begin()
    try:
        for fn, result in ((th, o), (bg, g)):
            for kw in (dict(n_win=-1), dict(ntime=-1), dict(nchan=-1), dict(vis=None), dict(flags=None), dict(out=None)):
                assert fn(**kw) == _lib.TRI_EINVAL, (fn.__name__, kw)
            assert b"" != lib.tri_last_error()
            assert fn(n_win=0) == _lib.TRI_OK and fn(ntime=0) == _lib.TRI_OK and fn(nchan=0) == _lib.TRI_OK  # empty
            for dt in (_lib.TRI_VIS_C128, _lib.TRI_VIS_F64, 17, -1):
                assert fn(dtype=dt) == _lib.TRI_EUNSUPPORTED
            assert fn(dtype=17, n_win=0) == _lib.TRI_EUNSUPPORTED        # a bad dtype is named before an empty shape
            assert fn(n_win=1 << 31, ntime=1, nchan=1) == _lib.TRI_EUNSUPPORTED
            assert b"pass fewer windows per call" in lib.tri_last_error()
            assert fn(n_win=1 << 20, ntime=1 << 30, nchan=1 << 30) == _lib.TRI_EUNSUPPORTED
            assert fn(ntime=1 << 31) == _lib.TRI_EUNSUPPORTED
            assert fn(work=None) == _lib.TRI_EWORKSPACE and fn(nbytes=need - 1) == _lib.TRI_EWORKSPACE
            for kw in (dict(work=v + 256), dict(work=f - 256), dict(work=result - need + 1)):
                assert fn(**kw) == _lib.TRI_EINVAL, (fn.__name__, kw)
        for kw in (dict(order=-1), dict(order=4), dict(ct=0.0), dict(ct=-1.0), dict(ct=nan), dict(ct=inf), dict(cf=0.0),
                   dict(cf=nan), dict(dt=-1), dict(dt=4), dict(df=4), dict(pt=0), dict(pt=33), dict(pf=0), dict(pf=33),
                   dict(rounds=0), dict(rounds=MAX_ROUNDS + 1), dict(ms=1), dict(ms=0), dict(ms=-3),
                   dict(out=v + 8), dict(out=v + 511), dict(out=f), dict(out=f + 63), dict(out=f - 63)):
            assert th(**kw) == _lib.TRI_EINVAL, kw
        assert th(dtype=17, rounds=0) == _lib.TRI_EINVAL                 # a bad argument is named before a bad dtype
        for kw in (dict(axis=-1), dict(axis=2), dict(pieces=0), dict(pieces=33), dict(degree=-1), dict(degree=4),
                   dict(out=v + 256), dict(out=f - 255), dict(out=f + 63)):
            assert bg(**kw) == _lib.TRI_EINVAL, kw
        # the line-length limit, before any launch and before the workspace is looked at
        big = MAX_LINE + 1
        assert th(n_win=1, ntime=1, nchan=big, order=0) == _lib.TRI_EUNSUPPORTED
        assert b"at most" in lib.tri_last_error()
        assert th(n_win=1, ntime=big, nchan=1, order=1) == _lib.TRI_EUNSUPPORTED
        assert th(n_win=1, ntime=big, nchan=1, order=3) == _lib.TRI_EUNSUPPORTED
        assert th(n_win=1, ntime=1, nchan=big, order=2) == _lib.TRI_EUNSUPPORTED
        assert th(n_win=1, ntime=1, nchan=big, order=3, nbytes=0) == _lib.TRI_EWORKSPACE      # not fitted: no limit
        assert th(n_win=1, ntime=big, nchan=1, order=2, nbytes=0) == _lib.TRI_EWORKSPACE
        assert bg(n_win=1, ntime=big, nchan=1, axis=0) == _lib.TRI_EUNSUPPORTED
        assert bg(n_win=1, ntime=1, nchan=big, axis=1) == _lib.TRI_EUNSUPPORTED
        assert bg(n_win=1, ntime=big, nchan=1, axis=1, nbytes=0) == _lib.TRI_EWORKSPACE
    finally:
        log = _lib.kernel_log_end()
    assert log == {}, log


# ---- the kernel table against the sources ----
def scan_pf_kernels():
    found = set()
    paths = sorted(glob.glob(os.path.join(ROOT, "tricolour_amd", "csrc", "steps", "polyfit", "*")))
    assert paths
    for path in paths:
        with open(path, encoding="utf-8") as fh:
            found.update(re.findall(r"__global__[\s\S]{0,200}?\b(k_\w+)\s*\(", fh.read()))
    return found


def test_kernel_table_lists_what_the_sources_hold():
    from test_route_ledger import scan_instances, scan_kernels
    assert scan_pf_kernels() == set(KERNELS)
    assert not set(KERNELS) & scan_kernels()                   # the ledger keeps the kernels directly under csrc/
    sites = scan_instances()                                   # launch sites of the host code, macros expanded
    for kernel, instances in KERNELS.items():
        assert sites.get(kernel) == instances, kernel
    with open(os.path.join(ROOT, "tricolour_amd", "csrc", "tricolour_amd.hip"), encoding="utf-8") as fh:
        hip = fh.read()
    assert '#include "steps/polyfit/kernels_polyfit.hpp"' in hip and '#include "steps/polyfit/polyfit_host.hpp"' in hip
    with open(os.path.join(ROOT, "tricolour_amd", "csrc", "steps", "polyfit", "kernels_polyfit.hpp"), encoding="utf-8") as fh:
        text = fh.read()
    for name, value in (("PF_CELL", CELL), ("PF_MAX_PIECES", MAX_PIECES), ("PF_MAX_LINE", MAX_LINE),
                        ("PF_MAX_ROUNDS", MAX_ROUNDS), ("PF_NT", 256)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
    assert "atomic" not in text.replace("No atomics", "") and "getenv" not in text


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
    MET.update(k for k in log if k.startswith("k_pf_"))


def kernels_of(log):
    return {k for k in log if k.startswith("k_pf_")}


_CACHE = {}


def expected(key, vis, flags, kw, bg):
    """The restatement's outputs: {order: out} and {axis: background}; computed once per key and left unchanged."""
    if key not in _CACHE:
        e = dict(restate(vis, flags, **kw))
        for axis, (pieces, degree) in bg.items():
            e["bg_" + axis] = restate_background(vis, flags, axis, pieces, degree)
        for v in e.values():
            v.setflags(write=False)
        _CACHE[key] = e
    return _CACHE[key]


def poisoned(torch, shape, dtype, fill):
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda").view(dtype).view(shape)


def c_entry_points(torch, v, f8, kw, bg, fill, out_offset=0):
    """{order: out} of tri_polyfit_threshold and {bg_axis: background} of tri_polyfit_background for device tensors,
    every output and the workspace full of `fill` bytes before each call; out_offset: bytes the flag output lies past an
    aligned address."""
    from tricolour_amd import _lib
    lib = _lib.lib()
    kw = dict(DEFAULTS, **kw)
    nbl, ncorr, T, F = v.shape
    n_win = nbl * ncorr
    code = _lib.TRI_VIS_C64 if v.dtype == torch.complex64 else _lib.TRI_VIS_F32
    stream = torch.cuda.current_stream().cuda_stream
    got = {}
    for o, order in enumerate(ORDERS):
        need = lib.tri_polyfit_workspace_bytes(n_win, T, F, kw["time_pieces"])
        ws = poisoned(torch, (need,), torch.uint8, fill)
        raw = poisoned(torch, (v.numel() + out_offset,), torch.uint8, fill)
        out = raw[out_offset:].view(v.shape)
        _lib.check(lib.tri_polyfit_threshold(v.data_ptr(), code, f8.data_ptr(), out.data_ptr(), n_win, T, F, o,
                                             kw["time_cutoff"], kw["time_degree"], kw["time_pieces"], kw["freq_cutoff"],
                                             kw["freq_degree"], kw["freq_pieces"], kw["rounds"], kw["min_samples"],
                                             ws.data_ptr(), need, stream))
        got[order] = out.cpu().numpy()
    for a, axis in enumerate(("time", "freq")):
        pieces, degree = bg[axis]
        need = lib.tri_polyfit_workspace_bytes(n_win, T, F, pieces if axis == "time" else 0)
        ws = poisoned(torch, (need,), torch.uint8, fill)
        out = poisoned(torch, v.shape, torch.float32, fill)
        _lib.check(lib.tri_polyfit_background(v.data_ptr(), code, f8.data_ptr(), n_win, T, F, a, pieces, degree,
                                              out.data_ptr(), ws.data_ptr(), need, stream))
        got["bg_" + axis] = out.cpu().numpy()
    return got


def check(key, vis, flags, container="tensor", offset=False, max_windows=None, abi=True, orders=ORDERS,
          axes=("time", "freq"), **kw):
    """threshold_polyfit in the given orders, polyfit_background along the given axes and (abi) the C entry points with
    poisoned outputs and workspace, against the restatement: the flags exactly, the background in every bit, the
    results' container and dtype, and the inputs unchanged."""
    import torch
    from tricolour_amd import flagging
    full = dict(DEFAULTS, **kw)
    bg = {"time": (full["time_pieces"], full["time_degree"]), "freq": (full["freq_pieces"], full["freq_degree"])}
    e = expected(key, vis, flags, kw, bg)
    extra = {} if max_windows is None else dict(_max_windows=max_windows)
    if container == "numpy":
        v, f = vis.copy(), flags.copy()
    else:
        v, f = dev(torch, vis, offset), dev(torch, flags, offset)
        if offset and vis.size:
            assert v.data_ptr() % 16 != 0 and f.data_ptr() % 4 != 0
        f0 = f.clone()
    got = {order: flagging.threshold_polyfit(v, f, order=order, **kw, **extra) for order in orders}
    got.update({"bg_" + axis: flagging.polyfit_background(v, f, axis, *bg[axis], **extra) for axis in axes})
    if container == "numpy":
        assert all(isinstance(x, np.ndarray) for x in got.values())
        assert same_bits(v, vis) and np.array_equal(f, flags)
    else:
        assert all(x.is_cuda for x in got.values())
        assert same_bits(v.cpu().numpy(), vis) and torch.equal(f, f0)
        got = {k: x.cpu().numpy() for k, x in got.items()}
    results = [("", got)]
    if abi:
        vd, fd = (dev(torch, vis), dev(torch, flags)) if container == "numpy" else (v, f)
        for fill in (0xFF, 0x00):
            results.append((" (C, fill %#x)" % fill, c_entry_points(torch, vd, fd.view(torch.uint8), kw, bg, fill)))
    for label, res in results:
        for name, g in res.items():
            if name.startswith("bg_"):
                assert g.dtype == np.float32 and g.shape == e[name].shape, (key, name, label)
                assert differing(g, e[name]) == 0, "%s: %d bit patterns of %s differ%s" % (key, differing(g, e[name]), name, label)
            else:
                if not label:
                    assert g.dtype == flags.dtype, (key, name, g.dtype)
                nbad = int(((g != 0) != e[name]).sum())
                assert g.shape == e[name].shape and nbad == 0, "%s: %d flags of order %s differ%s" % (key, nbad, name, label)
                assert set(np.unique(g.astype(np.uint8))) <= {0, 1}
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 1, 1, 7), (1, 1, 7, 1), (2, 1, 3, 5)])
def test_gpu_smallest_shapes(gpu, shape, dtype):
    with compared():
        vis, flags = make_case(shape, 1, dtype, "flags30" if shape[0] > 1 else "noise")
        check(("small", shape, dtype), vis, flags, min_samples=2, time_cutoff=1.0, freq_cutoff=1.0)
        check(("small-default", shape, dtype), vis, flags, abi=False)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("nchan", [31, 32, 33, 224, 230, 450])
def test_gpu_cell_and_piece_edges_along_frequency(gpu, nchan, dtype):
    """7 pieces: 224 = 7 x 32 has every piece edge on a cell edge, the others do not; 31 .. 33 straddle one cell."""
    with compared():
        vis, flags = make_case((2, 1, 9, nchan), 10 + nchan, dtype, "flags30" if nchan % 2 else "noise")
        e = check(("edges", nchan, dtype), vis, flags, freq_pieces=7, freq_cutoff=2.5, time_cutoff=3.0)
        assert e["freq"].sum() > (np.asarray(flags) != 0).sum()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("ntime", [33, 65])
def test_gpu_cell_and_piece_edges_along_time(gpu, ntime, dtype):
    with compared():
        vis, flags = make_case((2, 1, ntime, 21), 20 + ntime, dtype, "flags30" if ntime == 65 else "noise")
        e = check(("tedges", ntime, dtype), vis, flags, time_pieces=3, time_degree=2, time_cutoff=2.5)
        assert e["time"].sum() > (np.asarray(flags) != 0).sum()


# an aligned tensor of these channel counts: (prepare VEC, finish VEC)
CHANNELS = {230: (False, False), 228: (True, False), 224: (True, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("nchan", sorted(CHANNELS))
def test_gpu_channel_counts_and_offsets_pick_each_wide_load_instantiation(gpu, nchan, dtype):
    import torch
    vi = {"c64": 0, "f32": 1}[dtype]
    spell = lambda vec: "true" if vec else "false"
    vis, flags = make_case((2, 1, 5, nchan), 30, dtype, "flags30")
    vec_p, vec_f = CHANNELS[nchan]
    with compared() as log:
        check(("chan", nchan, dtype), vis, flags, abi=False, orders=("freqtime",), axes=())
    assert kernels_of(log) == {"k_pf_prepare<%d, %s>" % (vi, spell(vec_p)), "k_pf_finish<%s>" % spell(vec_f),
                               "k_pf_freq<4096, false>", "k_pf_time<false>"}, log
    if nchan == 224:
        # inputs one element past an aligned base: the scalar prepare pass, the same bits
        with compared() as log:
            check(("chan", nchan, dtype), vis, flags, abi=False, offset=True, orders=("freqtime",), axes=())
        assert "k_pf_prepare<%d, false>" % vi in log and "k_pf_finish<true>" in log, log
        # the flag output one byte past an aligned base: the scalar finish pass
        with compared() as log:
            e = expected(("chan", nchan, dtype), vis, flags, {}, {})
            got = c_entry_points(torch, dev(torch, vis), dev(torch, flags).view(torch.uint8), {},
                                 {"time": (1, 1), "freq": (7, 3)}, 0xFF, out_offset=1)
            for order in ORDERS:
                assert np.array_equal(got[order] != 0, e[order]), order
        assert "k_pf_finish<false>" in log and "k_pf_finish<true>" not in log, log


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("content", CONTENTS)
def test_gpu_contents(gpu, content, dtype):
    with compared():
        vis, flags = make_case((2, 2, 37, 70), 40 + CONTENTS.index(content), dtype, content)
        kw = dict(min_samples=2) if content == "truncate" else {}
        e = check((content, dtype), vis, flags, time_pieces=2, time_degree=3, **kw)
        if content in ("all_flagged", "constant", "ramp"):
            assert np.array_equal(e["freqtime"], flags) and np.array_equal(e["timefreq"], flags)
        if content == "few":
            assert np.array_equal(e["freq"], flags)            # no row reaches min_samples; the columns 0 .. 6 do
            assert np.isnan(e["bg_freq"]).any() and not np.isnan(e["bg_freq"]).all()
        if content == "all_flagged":
            assert np.isnan(e["bg_freq"]).all() and np.isnan(e["bg_time"]).all()
        if content in ("noise", "flags30", "huge", "tiny", "nonfinite"):
            assert e["freqtime"].sum() > (np.asarray(flags) != 0).sum()
            assert not np.array_equal(e["freqtime"], e["timefreq"])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_gpu_degrees(gpu, degree, dtype):
    with compared():
        vis, flags = make_case((2, 1, 40, 130), 60 + degree, dtype, "flags30")
        check(("degree", degree, dtype), vis, flags, time_degree=degree, freq_degree=degree, time_pieces=3, freq_pieces=5)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("rounds", [1, 5, 16])
def test_gpu_rounds(gpu, rounds, dtype):
    with compared():
        vis, flags = make_case((2, 1, 40, 130), 70, dtype, "noise")
        check(("rounds", rounds, dtype), vis, flags, rounds=rounds, time_pieces=32, freq_pieces=32, abi=rounds != 16)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
def test_gpu_degree_truncation_at_every_column(gpu, dtype):
    """Rows of 2, 3 and 4 adjacent usable channels in a single piece: the truncation fires at j = 1 and 2 in 2100
    channels and at j = 3 in 40; the same images transposed along time."""
    fired = set()
    with compared():
        for n in (2100, 40):
            vis, flags = make_case((1, 1, 6, n), 1, dtype, "truncate")
            av, valid = valid_of(vis[0, 0], flags[0, 0])
            fired |= set(truncated_at(fit(av, valid, 1, 3)[1], valid.sum(axis=1)[:, None], 3).reshape(-1))
            kw = dict(freq_pieces=1, time_pieces=1, time_degree=3, min_samples=2, freq_cutoff=0.5, time_cutoff=0.5, rounds=3)
            check(("truncate", n, dtype), vis, flags, abi=False, orders=("freq",), axes=("freq",), **kw)
            vt, ft = (np.ascontiguousarray(np.swapaxes(x, 2, 3)) for x in (vis, flags))
            check(("truncate-t", n, dtype), vt, ft, abi=False, orders=("time",), axes=("time",), **kw)
    assert fired == {0, 1, 2, 3}, fired


@pytest.mark.gpu
def test_gpu_more_pieces_than_samples(gpu):
    with compared():
        vis, flags = make_case((2, 1, 5, 9), 75, "c64", "noise")
        check("empty-pieces", vis, flags, time_pieces=7, freq_pieces=32, min_samples=2, time_cutoff=1.5, freq_cutoff=1.5)


@pytest.mark.gpu
def test_gpu_windows_are_isolated(gpu):
    """The middle window is 1e6 times the others: the outer windows' outputs are what they are when passed alone."""
    vis, flags = make_case((3, 1, 20, 70), 80, "c64", "flags30")
    vis[1] *= np.float32(1e6)
    with compared():
        e = check("isolated", vis, flags, abi=False)
        for w in (0, 2):
            alone = check(("isolated", w), vis[w:w + 1], flags[w:w + 1], abi=False)
            for name in alone:
                assert same_bits(alone[name][0], e[name][w]), (w, name)


@pytest.mark.gpu
def test_gpu_batching_gives_the_same_result(gpu):
    vis, flags = make_case((3, 2, 17, 36), 85, "c64", "flags30")
    with compared():
        check("batch", vis, flags, abi=False, time_pieces=2)
        check("batch", vis, flags, abi=False, time_pieces=2, max_windows=1)
        check("batch", vis, flags, abi=False, time_pieces=2, max_windows=4)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("container", ["numpy", "tensor"])
def test_gpu_containers(gpu, container, dtype):
    import torch
    from tricolour_amd import flagging
    vis, flags = make_case((2, 2, 9, 21), 90, dtype, "flags30")
    kw = dict(time_cutoff=2.0, freq_cutoff=2.0, min_samples=4)
    with compared():
        e = check(("containers", dtype), vis, flags, container=container, **kw)
        check(("containers", dtype), vis, flags, container=container, offset=container == "tensor", abi=False, **kw)
        assert e["freqtime"].sum() > flags.sum()
        # flags of another dtype, with values other than 1, come back in it as 0 / 1
        f8 = flags.astype(np.uint8) * 3
        args = (vis, f8) if container == "numpy" else (dev(torch, vis), dev(torch, f8))
        out = flagging.threshold_polyfit(*args, **kw)
        assert out.dtype == (np.uint8 if container == "numpy" else torch.uint8)
        assert np.array_equal(out if container == "numpy" else out.cpu().numpy(), e["freqtime"].astype(np.uint8))
        # non-contiguous inputs: a transposed view of (chan, time) storage
        vt, ft = np.ascontiguousarray(vis.swapaxes(2, 3)), np.ascontiguousarray(flags.swapaxes(2, 3))
        args = (vt, ft) if container == "numpy" else (dev(torch, vt), dev(torch, ft))
        args = tuple(a.swapaxes(2, 3) if container == "numpy" else a.transpose(2, 3) for a in args)
        out = flagging.threshold_polyfit(*args, **kw)
        assert np.array_equal(out if container == "numpy" else out.cpu().numpy(), e["freqtime"])


@pytest.mark.gpu
def test_gpu_lines_longer_than_the_small_lds_arrays(gpu):
    """4100 channels: the frequency pass with the large arrays; 4096: the last length of the small ones."""
    for nchan, want in ((SMALL_LINE + 4, "k_pf_freq<16384, %s>"), (SMALL_LINE, "k_pf_freq<4096, %s>")):
        vis, flags = make_case((1, 2, 3, nchan), 95, "c64", "flags30")
        with compared() as log:
            check(("long", nchan), vis, flags, abi=False, orders=("freq", "freqtime"), axes=("freq",))
        assert {want % "false", want % "true"} <= kernels_of(log), log


@pytest.mark.gpu
def test_gpu_longest_line_and_the_refusal_above_it(gpu):
    import torch
    from tricolour_amd import flagging
    with compared():
        vis, flags = make_case((1, 1, 2, MAX_LINE), 96, "f32", "noise")
        check("longest-freq", vis, flags, abi=False, orders=("freq",), axes=("freq",))
        vis, flags = make_case((1, 1, MAX_LINE, 3), 97, "f32", "noise")
        check("longest-time", vis, flags, abi=False, orders=("time",), axes=("time",), time_pieces=3, time_degree=2)
    from tricolour_amd import _lib
    _lib.kernel_log_begin()
    try:
        for shape, order, axis in (((1, 1, 1, MAX_LINE + 1), "freq", "freq"), ((1, 1, MAX_LINE + 1, 1), "time", "time"),
                                   ((1, 1, 1, MAX_LINE + 1), "timefreq", "freq")):
            v = torch.ones(shape, dtype=torch.float32, device="cuda")
            f = torch.zeros(shape, dtype=torch.bool, device="cuda")
            with pytest.raises(NotImplementedError, match="at most"):
                flagging.threshold_polyfit(v, f, order=order)
            with pytest.raises(NotImplementedError, match="at most"):
                flagging.polyfit_background(v, f, axis)
    finally:
        log = _lib.kernel_log_end()
    assert not kernels_of(log), log
    # the axis that is not fitted has no limit
    vis, flags = make_case((1, 1, MAX_LINE + 1, 2), 98, "f32", "noise")
    with compared():
        check("unfitted-axis", vis, flags, abi=False, orders=("freq",), axes=("freq",), min_samples=2, freq_cutoff=0.5)


@pytest.mark.gpu
def test_gpu_behaviour_on_the_device(gpu):
    """The behaviour input of the CPU test on the device."""
    vis, chan, row, blob = behaviour_input()
    with compared():
        e = check("behaviour", vis[None, None], np.zeros((1, 1) + vis.shape, bool))
    assert e["freqtime"][0, 0][chan].all() and e["freqtime"][0, 0][blob].all()


@pytest.mark.gpu
def test_gpu_every_listed_kernel_instantiation_was_launched_and_compared(gpu):
    """One compared call per dtype and route (the tests above add theirs when they ran): together they are the table."""
    for dtype in ("c64", "f32"):
        for nchan, offset in ((32, False), (20, False), (32, True), (21, False)):
            vis, flags = make_case((2, 1, 10, nchan), 110, dtype, "flags30")
            with compared():
                check(("routes", dtype, nchan), vis, flags, offset=offset, abi=False, min_samples=4)
    vis, flags = make_case((1, 1, 2, SMALL_LINE + 4), 111, "f32", "flags30")
    with compared():
        check("routes-long", vis, flags, abi=False, orders=("freq",), axes=("freq",))
    listed = set().union(*KERNELS.values())
    assert MET == listed, (sorted(listed - MET), sorted(MET - listed))
